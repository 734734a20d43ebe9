// lp_api.hip -- the extern "C" surface of liblightplane_hip.so (see include/lightplane_hip.h).
// Argument validation, kernel selection and error reporting; no device code here.
#include <stdarg.h>
#include <cmath>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lp_host.h"
#include "lp_mfma_common.h"
#if __has_include("build/lp_build_gen.h")
#include "build/lp_build_gen.h"  // written by build.py: LP_BUILD_SRC_HASH, LP_BUILD_FLAGS_JSON
#endif
#ifndef LP_BUILD_SRC_HASH
#define LP_BUILD_SRC_HASH "unknown (not built by lightplane_amd/csrc/build.py)"
#define LP_BUILD_FLAGS_JSON "null"
#endif

namespace lp {

static thread_local char g_err[512] = "";
thread_local uint32_t* g_relu_dump = nullptr;  // test hook, see lp_host.h
const char* volatile g_last_backward = "";

int set_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

// "<what>: <message>" -- or the bare message for the entry points that print no prefix (what == NULL: the Renderer, the Splatter)
static int fail(const char* what, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
static int fail(const char* what, int code, const char* fmt, ...) {
  int n = what ? snprintf(g_err, sizeof(g_err), "%s: ", what) : 0;
  if (n < 0 || n >= (int)sizeof(g_err)) n = 0;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err + n, sizeof(g_err) - n, fmt, ap);
  va_end(ap);
  return code;
}

int check_launch(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return LP_OK;
  return set_error((int)e, "%s: %s", what, hipGetErrorString(e));
}

static int64_t mlp_numel(const LpMlp& m) {
  int64_t n = 0;
  for (int l = 0; l < m.n_layers; ++l) n += (int64_t)m.dims[l] * m.dims[l + 1] + m.dims[l + 1];
  return n;
}

static int check_mlp(const char* name, const LpMlp& m, bool may_be_empty) {
  if (m.n_layers < 0 || m.n_layers > LP_MAX_LAYERS)
    return set_error(LP_EINVAL, "%s MLP: n_layers %d outside [0, %d]", name, m.n_layers, LP_MAX_LAYERS);
  if (m.n_layers == 0 && !may_be_empty) return set_error(LP_EINVAL, "%s MLP has no layers", name);
  for (int l = 0; l <= m.n_layers && m.n_layers > 0; ++l)
    if (m.dims[l] < 1 || m.dims[l] > LP_MAX_WIDTH)
      return set_error(LP_EUNSUPPORTED, "%s MLP: width %d of layer %d outside [1, %d]", name, m.dims[l], l,
                       LP_MAX_WIDTH);
  return LP_OK;
}

// What a grid-list has to satisfy beyond what every list does (n_grids and channels in range, positive extents, a non-negative
// row_offset, rows inside the flat tensor).
struct GridListRule {
  int min_grids;           // 0: the list may be absent (the colour grid-list)
  bool sampled;            // the samplers read it: every grid has two non-singular axes at least and the batch size of the first
  int row_cap_code;        // LP_OK: no cap; otherwise what a grid that ends at row 2^31 or beyond is refused with
  // the one wording that did not merge: tests/test_grid_tv_host.py holds the regulariser to "non-positive extent" and
  // tests/test_grid_resample_host.py the resampler to "empty extent" for the same defect
  const char* bad_extent;
};
// (the row cap is LP_EUNSUPPORTED for the regulariser and LP_EINVAL for the resampler: an accident of their history that callers may
// rely on by now -- the rule carries the code so that this file does not change it)
static const GridListRule SAMPLED = {1, true, LP_OK, "non-positive extent"};
static const GridListRule SAMPLED_OR_ABSENT = {0, true, LP_OK, "non-positive extent"};
static const GridListRule TV_LIST = {1, false, LP_EUNSUPPORTED, "non-positive extent"};
static const GridListRule RESAMPLE_LIST = {1, false, LP_EINVAL, "empty extent"};

// THE grid-list rule.  `label`: how messages name the list ("grid", "grid_tv: grid", "lp_grid_resample_forward: source grid").
static int check_grid_list(const char* label, const LpGridList& gl, const GridListRule& rule) {
  if (gl.n_grids < 0 || gl.n_grids > LP_MAX_GRIDS)
    return set_error(LP_EINVAL, "%s: n_grids %d outside [%d, %d]", label, gl.n_grids, rule.min_grids, LP_MAX_GRIDS);
  if (gl.n_grids == 0)
    return rule.min_grids == 0 ? LP_OK : set_error(LP_EINVAL, "%s: empty grid-list (n_grids 0 outside [1, %d])", label, LP_MAX_GRIDS);
  if (gl.channels < 1 || gl.channels > LP_MAX_WIDTH)
    return set_error(LP_EUNSUPPORTED, "%s: %d channels outside [1, %d]", label, gl.channels, LP_MAX_WIDTH);
  const int B = gl.grids[0].B;
  for (int g = 0; g < gl.n_grids; ++g) {
    const LpGrid& d = gl.grids[g];
    if (d.B < 1 || d.D < 1 || d.H < 1 || d.W < 1)
      return set_error(LP_EINVAL, "%s[%d]: %s [%d,%d,%d,%d]", label, g, rule.bad_extent, d.B, d.D, d.H, d.W);
    if (rule.sampled && d.B != B) return set_error(LP_EINVAL, "%s[%d]: batch %d != %d", label, g, d.B, B);
    const int ns = (d.D > 1) + (d.H > 1) + (d.W > 1);
    if (rule.sampled && ns < 2)
      return set_error(LP_EINVAL, "%s[%d]: Unexpected n non-singular dim of input grid (%d)", label, g, ns);
    if (d.row_offset < 0) return set_error(LP_EINVAL, "%s[%d]: negative row_offset", label, g);
    const int64_t end = d.row_offset + (int64_t)d.B * d.D * d.H * d.W;
    if (rule.row_cap_code != LP_OK && end >= ((int64_t)1 << 31))
      return set_error(rule.row_cap_code, "%s[%d] ends at row %lld: at most 2^31 - 1 rows per tensor", label, g, (long long)end);
    // a grid without its own pointer lives in the flat tensor: it has to fit
    if (!d.data && end > gl.n_rows)
      return set_error(LP_EINVAL, "%s[%d]: rows [%lld, %lld) outside the flat tensor (%lld rows)", label, g,
                       (long long)d.row_offset, (long long)end, (long long)gl.n_rows);
  }
  return LP_OK;
}

// every grid gets an explicit base pointer: its own (zero-copy list) or the flat tensor's
static bool normalize_grid_list(LpGridList& gl) {
  bool all = true;
  for (int g = 0; g < gl.n_grids; ++g) {
    if (!gl.grids[g].data) gl.grids[g].data = gl.data;
    all = all && gl.grids[g].data != nullptr;
  }
  for (int g = gl.n_grids > 0 ? gl.n_grids : 0; g < LP_MAX_GRIDS; ++g) gl.grids[g].data = nullptr;
  return all;
}
// gradient buffers: entry g = its own buffer or the flat one; either every grid has one or none has
static int normalize_grad_list(const char* name, float** list, float* flat, int n_grids) {
  int have = 0;
  for (int g = 0; g < LP_MAX_GRIDS; ++g) {
    if (g >= n_grids) { list[g] = nullptr; continue; }
    if (!list[g]) list[g] = flat;
    have += list[g] != nullptr;
  }
  if (have != 0 && have != n_grids)
    return set_error(LP_EINVAL, "%s: gradient buffers given for %d of %d grids (all or none)", name, have, n_grids);
  return LP_OK;
}

// Every non-NULL device pointer of an argument block is 16-byte aligned (lightplane_hip.h, Conventions): the kernels read and write
// caller memory as float4 / float2 and an under-aligned vector access is undefined.  One rule for every pointer, whatever n_rays is and
// whether today's kernels vectorise that field or not -- it cannot go stale when a kernel gains a vector access.  Host arithmetic only:
// runs before anything touches the device.  The message begins with the field as the header spells it.
static int check_aligned(const char* field, const void* p) {
  if (((uintptr_t)p & 15) == 0) return LP_OK;
  return set_error(LP_EINVAL, "%s = %p has to be 16-byte aligned (every device pointer of the ABI is)", field, p);
}
#define LP_ALIGNED(obj, field)                                        \
  do {                                                                \
    if (int rc_ = check_aligned(#field, (obj).field)) return rc_;     \
  } while (0)

// (row offsets inside the flat tensor are not pointers: a C % 4 != 0 list keeps the kernels' scalar path)
static int check_grid_list_aligned(const char* name, const LpGridList& gl) {
  char field[64];
  snprintf(field, sizeof(field), "%s.data", name);
  if (int rc = check_aligned(field, gl.data)) return rc;
  for (int g = 0; g < LP_MAX_GRIDS; ++g) {
    snprintf(field, sizeof(field), "%s.grids[%d].data", name, g);
    if (int rc = check_aligned(field, gl.grids[g].data)) return rc;
  }
  return LP_OK;
}

static int check_ptr_list_aligned(const char* name, float* const* list) {
  char field[64];
  for (int g = 0; g < LP_MAX_GRIDS; ++g) {
    snprintf(field, sizeof(field), "%s[%d]", name, g);
    if (int rc = check_aligned(field, list[g])) return rc;
  }
  return LP_OK;
}

// The five tensors every batch of rays brings: 16-byte aligned whatever n_rays is (`given` false), non-NULL when there are rays
// (`given` true).  Two calls, because every other pointer of a block is judged for alignment between the two.
static int check_ray_pointers(const char* what, const LpRays& r, bool given) {
  const struct { const char* field; const void* p; } ptrs[] = {
      {"rays.directions", r.directions}, {"rays.origins", r.origins}, {"rays.grid_idx", r.grid_idx},
      {"rays.near_t", r.near_t},         {"rays.far_t", r.far_t}};
  for (const auto& f : ptrs) {
    if (!given) {
      if (int rc = check_aligned(f.field, f.p)) return rc;
    } else if (r.n_rays > 0 && !f.p) {
      return fail(what, LP_ENULL, "rays: directions/origins/grid_idx/near/far must be non-NULL");
    }
  }
  return LP_OK;
}

static int check_rays(const LpRays& r, bool need_encoding) {
  int rc;
  if (r.n_rays < 0) return set_error(LP_EINVAL, "n_rays %lld < 0", (long long)r.n_rays);
  if ((rc = check_ray_pointers(nullptr, r, false))) return rc;
  if ((rc = check_aligned("rays.encoding", r.encoding))) return rc;
  if (r.n_rays == 0) return LP_OK;
  if ((rc = check_ray_pointers(nullptr, r, true))) return rc;
  if (need_encoding && !r.encoding) return set_error(LP_ENULL, "rays.encoding is NULL");
  if (r.row_length < 0) return set_error(LP_EINVAL, "rays.row_length %d < 0 (0 = unknown)", r.row_length);
  if (r.encoding_dim < 0 || r.encoding_dim > LP_MAX_WIDTH)
    return set_error(LP_EUNSUPPORTED, "rays.encoding_dim %d outside [0, %d]", r.encoding_dim, LP_MAX_WIDTH);
  return LP_OK;
}

static int check_march(const LpMarch& m) {
  if (m.num_samples < 1) return set_error(LP_EINVAL, "num_samples %d < 1", m.num_samples);
  if (m.num_samples_inf < 0) return set_error(LP_EINVAL, "num_samples_inf %d < 0", m.num_samples_inf);
  return LP_OK;
}

// The decoder rule (Renderer, scaffold, decoder at points) in three parts.  First the trunk and the opacity head: the trunk reads the
// grid's C channels, the heads read the trunk's output (`head_in`; C without a trunk), the opacity head ends in one output, and the two
// lie trunk|opacity at the start of mlp_params.
static int check_trunk_and_opacity(const char* what, int C, const LpMlp& trunk, const LpMlp& opacity, int& head_in) {
  int rc;
  if ((rc = check_mlp("trunk", trunk, true))) return rc;
  if ((rc = check_mlp("opacity", opacity, false))) return rc;
  head_in = C;
  if (trunk.n_layers > 0) {
    if (trunk.dims[0] != C) return fail(what, LP_EINVAL, "trunk MLP input width %d != grid channels %d", trunk.dims[0], C);
    head_in = trunk.dims[trunk.n_layers];
  }
  if (opacity.dims[0] != head_in) return fail(what, LP_EINVAL, "opacity MLP input width %d != %d", opacity.dims[0], head_in);
  if (opacity.dims[opacity.n_layers] != 1)
    return fail(what, LP_EINVAL, "opacity MLP must end in 1 output, got %d", opacity.dims[opacity.n_layers]);
  if (trunk.offset != 0 || opacity.offset != mlp_numel(trunk))
    return fail(what, LP_EINVAL, "MLP offsets do not follow the trunk|opacity|color flat layout");
  return LP_OK;
}

// ... then the colour head, where the block has one: it reads `head_in` too and follows the opacity head in mlp_params (`offset`).
// `runs`: it is evaluated, so it has to exist, color_chn is one of its outputs and the encoding has its input width.
static int check_color_head(const char* what, const LpMlp& color, int head_in, int64_t offset, bool runs, int color_chn, int encoding_dim) {
  if (int rc = check_mlp("color", color, !runs)) return rc;
  if (color.n_layers > 0) {
    if (color.dims[0] != head_in) return fail(what, LP_EINVAL, "colour MLP input width %d != %d", color.dims[0], head_in);
    if (color.offset != offset) return fail(what, LP_EINVAL, "MLP offsets do not follow the trunk|opacity|color flat layout");
  }
  if (!runs) return LP_OK;
  if (color_chn < 1 || color_chn > color.dims[color.n_layers])
    return fail(what, LP_EINVAL, "color_chn %d outside [1, %d]", color_chn, color.dims[color.n_layers]);
  if (encoding_dim != head_in) return fail(what, LP_EINVAL, "encoding_dim %d != the colour head's input width %d", encoding_dim, head_in);
  return LP_OK;
}

static int bad_param_count(int64_t expect, int64_t got) {  // (the reference's wording)
  return set_error(LP_EINVAL, "The number of elements in mlp param should be %lld. Got %lld instead.", (long long)expect, (long long)got);
}

// ... and mlp_params holds them: `exact` -- the Renderer, as the reference -- and nothing else
static int check_param_count(const char* what, int64_t need, int64_t n_mlp_params, bool exact) {
  if (exact && need != n_mlp_params) return bad_param_count(need, n_mlp_params);
  if (need > n_mlp_params)
    return fail(what, LP_EINVAL, "the MLPs take %lld floats, mlp_params has %lld", (long long)need, (long long)n_mlp_params);
  return LP_OK;
}

// a separate colour grid-list mirrors the grid-list, and its decoder has no trunk
static int check_color_grid(const char* what, const LpGridList& grid, const LpGridList& color_grid, const LpMlp& trunk) {
  if (color_grid.n_grids == 0) return LP_OK;
  if (color_grid.channels != grid.channels || color_grid.grids[0].B != grid.grids[0].B)
    return fail(what, LP_EINVAL, "color_grid must share batch size and channel count with grid");
  if (trunk.n_layers != 0) return fail(what, LP_EINVAL, "the trunk MLP has to have 0 layers with a separate colour grid-list");
  return LP_OK;
}

// a [B, D, H, W] shape (`name`: "scaffold", "volume") has positive extents
static int check_shape(const char* what, const char* name, const LpGrid& s) {
  if (s.B < 1 || s.D < 1 || s.H < 1 || s.W < 1)
    return fail(what, LP_EINVAL, "%s shape [%d,%d,%d,%d] has an extent < 1", name, s.B, s.D, s.H, s.W);
  return LP_OK;
}

// the scaffold a sampler looks samples up in: a shape, and one scene per scene of the grid-list
static int check_scaffold_for_grid(const char* what, const LpGrid& s, const LpGridList& grid) {
  if (int rc = check_shape(what, "scaffold", s)) return rc;
  if (s.B != grid.grids[0].B)
    return fail(what, LP_EINVAL, "scaffold shape [%d,%d,%d,%d] incompatible with grid batch %d", s.B, s.D, s.H, s.W, grid.grids[0].B);
  return LP_OK;
}

// a batch of n_rays x n_pts points: one wavefront per 64 of them, and a launch has at most 2^31 workgroups.  `below_2_31`: the kernels
// index the points themselves with 32 bits (the march in pieces, one wavefront per ray), so their number has to stay below 2^31.
static int check_point_batch(const char* what, int64_t n_rays, int64_t n_pts, bool below_2_31 = false) {
  if (n_rays < 0 || n_pts < 0) return fail(what, LP_EINVAL, "n_rays %lld / n_pts %lld < 0", (long long)n_rays, (long long)n_pts);
  if (below_2_31 && n_pts > 0 && n_rays > (((int64_t)1 << 31) - 1) / n_pts)
    return fail(what, LP_EUNSUPPORTED, "n_rays %lld x %lld samples per ray: has to stay below 2^31", (long long)n_rays, (long long)n_pts);
  if (n_pts > 0 && n_rays > (((int64_t)1 << 37) - 64) / n_pts)
    return fail(what, LP_EUNSUPPORTED, "%lld x %lld points are more than 2^31 wavefronts", (long long)n_rays, (long long)n_pts);
  return LP_OK;
}

// THE workspace rule: there, as large as `query`() -- the entry point's *_workspace_bytes -- asks for, and aligned.  (A NULL workspace
// is LP_EINVAL for lp_scaffold_build and LP_ENULL everywhere else: `null_code` keeps what callers see.)
static int check_workspace(const char* what, const char* query, const void* workspace, int64_t workspace_bytes, int64_t need, int align,
                           int null_code) {
  if (!workspace) return fail(what, null_code, "workspace is NULL, %s() asks for %lld bytes", query, (long long)need);
  if (workspace_bytes < need)
    return fail(what, LP_EINVAL, "workspace of %lld bytes, %s() asks for %lld", (long long)workspace_bytes, query, (long long)need);
  if (((uintptr_t)workspace & (uintptr_t)(align - 1)) != 0)
    return fail(what, LP_EINVAL, "workspace = %p has to be %d-byte aligned", workspace, align);
  return LP_OK;
}

// [n_rays][S_tot][w] words of a ReLU dump
static int check_dump_words(const LpRays& rays, const LpMarch& m, int w, int64_t dump_words) {
  const int64_t want = rays.n_rays * (int64_t)(m.num_samples + m.num_samples_inf) * w;
  if (dump_words != want)
    return set_error(LP_EINVAL, "relu dump: %lld words given, [n_rays][S_tot][%d] = %lld needed", (long long)dump_words, w, (long long)want);
  return LP_OK;
}

static int check_renderer(const LpRendererArgs& a, bool backward) {
  int rc;
  if ((rc = check_rays(a.rays, true))) return rc;
  if ((rc = check_grid_list_aligned("grid", a.grid))) return rc;
  if ((rc = check_grid_list_aligned("color_grid", a.color_grid))) return rc;
  LP_ALIGNED(a, scaffold);
  LP_ALIGNED(a, scaffold_shape.data);
  LP_ALIGNED(a, mlp_params);
  LP_ALIGNED(a, ray_length);
  LP_ALIGNED(a, neg_log_t);
  LP_ALIGNED(a, feature);
  LP_ALIGNED(a, neg_log_t_ckpt);
  LP_ALIGNED(a, grad_ray_length);
  LP_ALIGNED(a, grad_neg_log_t);
  LP_ALIGNED(a, grad_feature);
  LP_ALIGNED(a, grad_grid);
  LP_ALIGNED(a, grad_color_grid);
  LP_ALIGNED(a, grad_mlp_params);
  LP_ALIGNED(a, grad_encoding);
  if ((rc = check_ptr_list_aligned("grad_grid_list", a.grad_grid_list))) return rc;
  if ((rc = check_ptr_list_aligned("grad_color_grid_list", a.grad_color_grid_list))) return rc;
  LP_ALIGNED(a, bg_color);
  LP_ALIGNED(a, alpha);
  LP_ALIGNED(a, grad_alpha);
  LP_ALIGNED(a, seg_prefix);
  if ((rc = check_march(a.march))) return rc;
  if ((rc = check_grid_list("grid", a.grid, SAMPLED))) return rc;
  if ((rc = check_grid_list("color_grid", a.color_grid, SAMPLED_OR_ABSENT))) return rc;
  if ((rc = check_color_grid(nullptr, a.grid, a.color_grid, a.trunk))) return rc;
  if (!(a.stop_neg_log_t >= 0.0f)) return set_error(LP_EINVAL, "stop_neg_log_t must be >= 0 (0 = no early termination)");
  if (a.arithmetic != LP_ARITH_DEFAULT && a.arithmetic != LP_ARITH_FP32)
    return set_error(LP_EINVAL, "arithmetic %d is neither LP_ARITH_DEFAULT nor LP_ARITH_FP32", a.arithmetic);
  if (a.march_order != LP_MARCH_RAYS_PER_WAVE && a.march_order != LP_MARCH_SAMPLES_PER_WAVE)
    return set_error(LP_EINVAL, "march_order %d is neither LP_MARCH_RAYS_PER_WAVE nor LP_MARCH_SAMPLES_PER_WAVE", a.march_order);
  if (backward && a.stop_neg_log_t > 0.0f && !a.neg_log_t_ckpt)
    return set_error(LP_ENULL, "early termination needs neg_log_t_ckpt in the backward (it records where the forward stopped)");
  int head_in;
  if ((rc = check_trunk_and_opacity(nullptr, a.grid.channels, a.trunk, a.opacity, head_in))) return rc;
  const int64_t n_to = mlp_numel(a.trunk) + mlp_numel(a.opacity);
  if ((rc = check_color_head(nullptr, a.color, head_in, n_to, true, a.color_chn, a.rays.encoding_dim))) return rc;
  if ((rc = check_param_count(nullptr, n_to + mlp_numel(a.color), a.n_mlp_params, true))) return rc;
  if (!a.mlp_params) return set_error(LP_ENULL, "mlp_params is NULL");
  if (a.scaffold && (rc = check_scaffold_for_grid(nullptr, a.scaffold_shape, a.grid))) return rc;
  if (a.rays.n_rays > 0) {
    if (!backward && (!a.ray_length || !a.neg_log_t || !a.feature))
      return set_error(LP_ENULL, "forward outputs (ray_length, neg_log_t, feature) must be non-NULL");
    if (backward && !a.neg_log_t)
      return set_error(LP_ENULL, "backward needs neg_log_t saved by the forward pass");
  }
  return LP_OK;
}

static int check_splatter(const LpSplatterArgs& a, bool backward) {
  int rc;
  if (a.march_order != LP_MARCH_RAYS_PER_WAVE && a.march_order != LP_MARCH_SAMPLES_PER_WAVE)
    return set_error(LP_EINVAL, "march_order %d is neither LP_MARCH_RAYS_PER_WAVE nor LP_MARCH_SAMPLES_PER_WAVE", a.march_order);
  if ((rc = check_rays(a.rays, true))) return rc;
  if ((rc = check_grid_list_aligned("out", a.out))) return rc;
  if ((rc = check_grid_list_aligned("input_grid", a.input_grid))) return rc;
  LP_ALIGNED(a, out_feature);
  LP_ALIGNED(a, out_weight);
  LP_ALIGNED(a, mlp_params);
  LP_ALIGNED(a, grad_out);
  LP_ALIGNED(a, weight);
  LP_ALIGNED(a, grad_encoding);
  LP_ALIGNED(a, grad_input_grid);
  LP_ALIGNED(a, grad_mlp_params);
  if ((rc = check_ptr_list_aligned("grad_input_grid_list", a.grad_input_grid_list))) return rc;
  if ((rc = check_march(a.march))) return rc;
  if ((rc = check_grid_list("out", a.out, SAMPLED))) return rc;
  const bool use_mlp = a.mlp.n_layers > 0;
  if (use_mlp) {
    // MLP-Splatter: MLP(sample(input_grid) + encoding) is splatted (reference lightplane_splatter.py:167-338)
    if ((rc = check_mlp("splatter", a.mlp, false))) return rc;
    if ((rc = check_grid_list("input_grid", a.input_grid, SAMPLED))) return rc;
    if (a.input_grid.grids[0].B != a.out.grids[0].B)
      return set_error(LP_EINVAL, "input_grid batch %d != output grid batch %d", a.input_grid.grids[0].B,
                       a.out.grids[0].B);
    if (a.mlp.dims[0] != a.input_grid.channels || a.mlp.dims[0] != a.rays.encoding_dim)
      return set_error(LP_EINVAL, "MLP input width %d must equal input_grid channels %d and encoding width %d",
                       a.mlp.dims[0], a.input_grid.channels, a.rays.encoding_dim);
    if (a.mlp.dims[a.mlp.n_layers] != a.out.channels)
      return set_error(LP_EINVAL, "MLP output width %d != output grid channels %d", a.mlp.dims[a.mlp.n_layers],
                       a.out.channels);
    if (a.mlp.offset != 0 || mlp_numel(a.mlp) != a.n_mlp_params) return bad_param_count(mlp_numel(a.mlp), a.n_mlp_params);
    if (!a.mlp_params) return set_error(LP_ENULL, "mlp_params is NULL");
  } else if (a.rays.encoding_dim != a.out.channels) {
    return set_error(LP_EINVAL, "splatting feature width %d != output grid channels %d", a.rays.encoding_dim,
                     a.out.channels);
  }
  if (a.rays.n_rays > 0) {
    if (!backward && (!a.out_feature || !a.out_weight))
      return set_error(LP_ENULL, "out_feature / out_weight must be non-NULL");
    if (backward && (!a.grad_out || !a.weight))
      return set_error(LP_ENULL, "grad_out / weight must be non-NULL");
    if (backward && !use_mlp && !a.grad_encoding) return set_error(LP_ENULL, "grad_encoding must be non-NULL");
  }
  return LP_OK;
}

// Grid-list of the total-variation regulariser (lp_grid_tv_*): any [B, D, H, W] with positive extents -- a line or a single cell is
// a valid (if dull) grid here, unlike for the samplers -- and grids of one list may differ in batch size; every tensor below 2^31 rows.
static int check_tv_grid_list(const LpGridList* gl) {
  if (!gl) return set_error(LP_ENULL, "grid_tv: the grid-list is NULL");
  return check_grid_list("grid_tv: grid", *gl, TV_LIST);
}

// everything lp_grid_tv_forward / _backward / _fused share; fills the normalised list and the per-grid gradient pointers
static int check_grid_tv(const char* what, const LpGridList* grid, const float* grid_weights, int n_weights, int p, bool want_loss,
                         float* loss, void* workspace, int64_t workspace_bytes, bool want_grad, float* grad, float* const* grad_list,
                         int n_grad_list, LpGridList& gl, float** grads) {
  int rc;
  if ((rc = check_tv_grid_list(grid))) return rc;
  if (p != 1 && p != 2) return set_error(LP_EINVAL, "%s: p = %d, has to be 1 (|d|) or 2 (d^2)", what, p);
  if (grid_weights ? n_weights != grid->n_grids : n_weights != 0)
    return set_error(LP_EINVAL, "%s: %d grid weights for %d grids (NULL / 0 = all 1)", what, n_weights, grid->n_grids);
  gl = *grid;
  if (!normalize_grid_list(gl)) return set_error(LP_ENULL, "%s: a grid has neither its own data pointer nor a flat tensor", what);
  if (want_loss) {
    if (!loss) return set_error(LP_ENULL, "%s: loss is NULL", what);
    if ((rc = check_workspace(what, "lp_grid_tv_workspace_bytes", workspace, workspace_bytes, grid_tv_workspace_bytes(gl), 8, LP_ENULL)))
      return rc;  // (doubles: 8-byte aligned)
  }
  if (want_grad) {
    if (grad_list ? (n_grad_list != gl.n_grids) : (n_grad_list != 0))
      return set_error(LP_EINVAL, "%s: gradient list of %d entries for %d grids", what, n_grad_list, gl.n_grids);
    if (!grad && !grad_list) return set_error(LP_ENULL, "%s: neither a flat gradient tensor nor a gradient list", what);
    for (int g = 0; g < gl.n_grids; ++g) {
      grads[g] = grad_list ? grad_list[g] : nullptr;
      // as for the Renderer's grad_grid_list: a grid without its own entry takes the flat buffer -- which mirrors the flat TENSOR, so
      // only a grid that lives there can use it
      if (!grads[g] && !grid->grids[g].data) grads[g] = grad;
      if (!grads[g])
        return set_error(LP_EINVAL, "%s: the gradient list does not match the grid list: no gradient buffer for grid %d%s", what, g,
                         grid->grids[g].data ? " (it has its own data pointer and needs its own gradient entry)" : "");
      if (grads[g] == gl.grids[g].data) return set_error(LP_EINVAL, "%s: the gradient of grid %d aliases the grid", what, g);
    }
  }
  return LP_OK;
}

// One list of lp_grid_resample_*: any positive extents, as for the regulariser; every tensor below 2^31 rows.
static int check_resample_list(const char* what, const char* name, const LpGridList* gl) {
  if (!gl) return set_error(LP_ENULL, "%s: the %s grid-list is NULL", what, name);
  char label[96];
  snprintf(label, sizeof(label), "%s: %s grid", what, name);
  return check_grid_list(label, *gl, RESAMPLE_LIST);
}

// everything lp_grid_resample_forward / _backward check; fills the normalised lists
static int check_grid_resample(const char* what, const LpGridList* src, const LpGridList* dst, int align_corners, const float* coeffs,
                               LpGridList& s, LpGridList& d) {
  int rc;
  if ((rc = check_resample_list(what, "source", src))) return rc;
  if ((rc = check_resample_list(what, "destination", dst))) return rc;
  if (src->n_grids != dst->n_grids)
    return set_error(LP_EINVAL, "%s: %d source grids for %d destination grids", what, src->n_grids, dst->n_grids);
  if (src->channels != dst->channels)
    return set_error(LP_EINVAL, "%s: %d source channels for %d destination channels", what, src->channels, dst->channels);
  for (int g = 0; g < src->n_grids; ++g)
    if (src->grids[g].B != dst->grids[g].B)
      return set_error(LP_EINVAL, "%s: grid[%d]: batch size %d of the source, %d of the destination (the batch axis is not resampled)",
                       what, g, src->grids[g].B, dst->grids[g].B);
  if (align_corners != 0 && align_corners != 1) return set_error(LP_EINVAL, "%s: align_corners = %d, has to be 0 or 1", what, align_corners);
  if (coeffs)
    for (int i = 0; i < 3 * src->n_grids; ++i)
      if (!(coeffs[i] > 0.0f) || !std::isfinite(coeffs[i]))
        return set_error(LP_EINVAL, "%s: coordinate coefficient %d (grid %d, axis %c) is %g: has to be finite and positive", what, i, i / 3,
                         "DHW"[i % 3], (double)coeffs[i]);
  s = *src, d = *dst;
  if (!normalize_grid_list(s) || !normalize_grid_list(d))
    return set_error(LP_ENULL, "%s: a grid has neither its own data pointer nor a flat tensor", what);
  const int64_t C = s.channels;
  for (int g = 0; g < s.n_grids; ++g)
    if ((((uintptr_t)s.grids[g].data | (uintptr_t)d.grids[g].data) & 3) != 0)
      return set_error(LP_EINVAL, "%s: grid[%d]: fp32 data has to be 4-byte aligned", what, g);
  for (int i = 0; i < s.n_grids; ++i) {
    const LpGrid& a = s.grids[i];
    const uintptr_t a0 = (uintptr_t)(a.data + a.row_offset * C), a1 = a0 + (uintptr_t)((int64_t)a.B * a.D * a.H * a.W * C * 4);
    for (int j = 0; j < d.n_grids; ++j) {
      const LpGrid& b = d.grids[j];
      const uintptr_t b0 = (uintptr_t)(b.data + b.row_offset * C), b1 = b0 + (uintptr_t)((int64_t)b.B * b.D * b.H * b.W * C * 4);
      if (a0 < b1 && b0 < a1) return set_error(LP_EINVAL, "%s: source grid %d aliases destination grid %d", what, i, j);
    }
  }
  return LP_OK;
}

// shape and dilation of a scaffold: all lp_scaffold_workspace_bytes() looks at
static int check_scaffold_shape(const char* what, const LpScaffoldArgs* args) {
  if (!args) return set_error(LP_ENULL, "%s: args is NULL", what);
  if (int rc = check_shape(what, "scaffold", args->shape)) return rc;
  if (args->dilate < 0) return set_error(LP_EINVAL, "%s: dilate = %d, has to be >= 0", what, args->dilate);
  return LP_OK;
}

// everything lp_scaffold_opacity / lp_scaffold_build share; fills the normalised copy
static int check_scaffold(const char* what, const LpScaffoldArgs* args, const float* out, LpScaffoldArgs& a) {
  int rc;
  if ((rc = check_scaffold_shape(what, args))) return rc;
  if ((rc = check_grid_list_aligned("grid", args->grid))) return rc;
  LP_ALIGNED(*args, mlp_params);
  if ((rc = check_aligned("scaffold / opacity (the result)", out))) return rc;
  if ((rc = check_grid_list("grid", args->grid, SAMPLED))) return rc;
  if (args->shape.B != args->grid.grids[0].B)
    return set_error(LP_EINVAL, "%s: scaffold batch %d != grid batch %d", what, args->shape.B, args->grid.grids[0].B);
  if (args->threshold != args->threshold) return set_error(LP_EINVAL, "%s: threshold is NaN", what);
  int head_in;
  if ((rc = check_trunk_and_opacity(what, args->grid.channels, args->trunk, args->opacity, head_in))) return rc;
  if ((rc = check_param_count(what, mlp_numel(args->trunk) + mlp_numel(args->opacity), args->n_mlp_params, false))) return rc;
  if (!args->mlp_params) return set_error(LP_ENULL, "%s: mlp_params is NULL", what);
  if (!out) return set_error(LP_ENULL, "%s: the result pointer is NULL", what);
  a = *args;
  if (!normalize_grid_list(a.grid)) return set_error(LP_ENULL, "%s: grid.data is NULL (and a grid has no pointer of its own)", what);
  return LP_OK;
}

// everything lp_points_forward / lp_points_backward share; fills the normalised copy.  `color`: the colour head takes part (forward:
// color_out given; backward: grad_color given) -- only then are the colour MLP, the colour grid-list's data and the encoding looked at.
static int check_points(const char* what, const LpPointsArgs* args, bool backward, LpPointsArgs& a) {
  int rc;
  if (!args) return set_error(LP_ENULL, "%s: args is NULL", what);
  const bool color = backward ? args->grad_color != nullptr : args->color_out != nullptr;
  if ((rc = check_grid_list_aligned("grid", args->grid))) return rc;
  if ((rc = check_grid_list_aligned("color_grid", args->color_grid))) return rc;
  LP_ALIGNED(*args, mlp_params);
  LP_ALIGNED(*args, points);
  LP_ALIGNED(*args, grid_idx);
  LP_ALIGNED(*args, encoding);
  LP_ALIGNED(*args, scaffold);
  LP_ALIGNED(*args, opacity_out);
  LP_ALIGNED(*args, color_out);
  LP_ALIGNED(*args, grad_opacity);
  LP_ALIGNED(*args, grad_color);
  LP_ALIGNED(*args, grad_grid);
  LP_ALIGNED(*args, grad_color_grid);
  if ((rc = check_ptr_list_aligned("grad_grid_list", args->grad_grid_list))) return rc;
  if ((rc = check_ptr_list_aligned("grad_color_grid_list", args->grad_color_grid_list))) return rc;
  LP_ALIGNED(*args, grad_mlp_params);
  LP_ALIGNED(*args, grad_encoding);
  LP_ALIGNED(*args, grad_points);
  if ((rc = check_point_batch(what, args->n_rays, args->n_pts))) return rc;
  if ((rc = check_grid_list("grid", args->grid, SAMPLED))) return rc;
  if ((rc = check_grid_list("color_grid", args->color_grid, SAMPLED_OR_ABSENT))) return rc;
  if ((rc = check_color_grid(what, args->grid, args->color_grid, args->trunk))) return rc;
  int head_in;
  if ((rc = check_trunk_and_opacity(what, args->grid.channels, args->trunk, args->opacity, head_in))) return rc;
  const int64_t n_to = mlp_numel(args->trunk) + mlp_numel(args->opacity);
  if ((rc = check_color_head(what, args->color, head_in, n_to, color, args->color_chn, args->encoding_dim))) return rc;
  if ((rc = check_param_count(what, n_to + mlp_numel(args->color), args->n_mlp_params, false))) return rc;
  if (args->scaffold && (rc = check_scaffold_for_grid(what, args->scaffold_shape, args->grid))) return rc;
  if (!args->mlp_params) return set_error(LP_ENULL, "%s: mlp_params is NULL", what);
  if (args->n_rays > 0 && args->n_pts > 0) {  // (an empty batch has no tensors to point at)
    if (!args->points || !args->grid_idx) return set_error(LP_ENULL, "%s: points / grid_idx is NULL", what);
    if (color && !args->encoding) return set_error(LP_ENULL, "%s: encoding is NULL and the colour head is evaluated", what);
    if (!backward && !args->opacity_out) return set_error(LP_ENULL, "%s: opacity_out is NULL", what);
  }
  a = *args;
  if (!normalize_grid_list(a.grid)) return set_error(LP_ENULL, "%s: grid.data is NULL (and a grid has no pointer of its own)", what);
  if (color && !normalize_grid_list(a.color_grid))
    return set_error(LP_ENULL, "%s: color_grid.data is NULL (and a grid has no pointer of its own)", what);
  if (backward) {
    if ((rc = normalize_grad_list("grad_grid", a.grad_grid_list, a.grad_grid, a.grid.n_grids))) return rc;
    if ((rc = normalize_grad_list("grad_color_grid", a.grad_color_grid_list, a.grad_color_grid, a.color_grid.n_grids))) return rc;
    const int total = points_backward_total_width(a);
    if (total > 1024) return set_error(LP_EUNSUPPORTED, "%s: sum of layer widths %d exceeds 1024", what, total);
  }
  return LP_OK;
}

// everything the four lp_point_* entry points check; fills the normalised copy.  mode: 0 gather, 1 splat, 2 normalize, 3 grad_points
static int check_point_grid(const char* what, const LpPointGridArgs* args, int mode, LpPointGridArgs& a) {
  int rc;
  if (!args) return set_error(LP_ENULL, "%s: args is NULL", what);
  if ((rc = check_grid_list_aligned("grid", args->grid))) return rc;
  if ((rc = check_ptr_list_aligned("row_weight", args->row_weight))) return rc;
  LP_ALIGNED(*args, points);
  LP_ALIGNED(*args, grid_idx);
  LP_ALIGNED(*args, vectors);
  LP_ALIGNED(*args, out_features);
  LP_ALIGNED(*args, grad_points);
  if ((rc = check_point_batch(what, args->n_rays, args->n_pts))) return rc;
  if ((rc = check_grid_list("grid", args->grid, SAMPLED))) return rc;
  if (args->channels != args->grid.channels)
    return set_error(LP_EINVAL, "%s: channels %d of the per-point vectors != grid channels %d", what, args->channels, args->grid.channels);
  int have = 0;
  for (int g = 0; g < args->grid.n_grids; ++g) have += args->row_weight[g] != nullptr;
  if (mode == 1 && have != 0 && have != args->grid.n_grids)
    return set_error(LP_EINVAL, "%s: row_weight given for %d of %d grids (all or none)", what, have, args->grid.n_grids);
  if (mode == 2 && have != args->grid.n_grids)
    return set_error(LP_ENULL, "%s: row_weight is NULL for %d of %d grids", what, args->grid.n_grids - have, args->grid.n_grids);
  if (mode != 2 && args->n_rays > 0 && args->n_pts > 0) {  // (an empty batch has no tensors to point at)
    if (!args->points || !args->grid_idx) return set_error(LP_ENULL, "%s: points / grid_idx is NULL", what);
    if (mode == 0 && !args->out_features) return set_error(LP_ENULL, "%s: out_features is NULL", what);
    if (mode != 0 && !args->vectors) return set_error(LP_ENULL, "%s: vectors is NULL", what);
    if (mode == 3 && !args->grad_points) return set_error(LP_ENULL, "%s: grad_points is NULL", what);
  }
  a = *args;
  if (!normalize_grid_list(a.grid)) return set_error(LP_ENULL, "%s: grid.data is NULL (and a grid has no pointer of its own)", what);
  for (int g = a.grid.n_grids; g < LP_MAX_GRIDS; ++g) a.row_weight[g] = nullptr;
  return LP_OK;
}

// everything lp_rays_clip checks
static int check_ray_clip(const LpRayClipArgs* args, const float* near_out, const float* far_out, const uint8_t* hit_out) {
  if (!args) return set_error(LP_ENULL, "lp_rays_clip: args is NULL");
  int rc;
  if (args->rays.n_rays < 0) return set_error(LP_EINVAL, "lp_rays_clip: n_rays %lld < 0", (long long)args->rays.n_rays);
  if ((rc = check_ray_pointers("lp_rays_clip", args->rays, false))) return rc;
  LP_ALIGNED(*args, scaffold);
  if ((rc = check_aligned("near_out", near_out)) || (rc = check_aligned("far_out", far_out))) return rc;
  if (!(args->pad >= 0.0f) || args->pad > 3.4028234663852886e38f)
    return set_error(LP_EINVAL, "lp_rays_clip: pad = %g, has to be >= 0 and finite", (double)args->pad);
  if (args->scaffold) {
    const LpGrid& s = args->scaffold_shape;
    if ((rc = check_shape("lp_rays_clip", "scaffold", s))) return rc;
    if ((int64_t)s.D + s.H + s.W >= ((int64_t)1 << 30))
      return set_error(LP_EUNSUPPORTED, "lp_rays_clip: scaffold shape [%d,%d,%d,%d]: D + H + W has to stay below 2^30", s.B, s.D, s.H, s.W);
  }
  if (!near_out || !far_out || !hit_out) return set_error(LP_ENULL, "lp_rays_clip: near_out / far_out / hit_out must be non-NULL");
  return check_ray_pointers("lp_rays_clip", args->rays, true);
}

// the shape of a lattice to mesh: all lp_mesh_workspace_bytes() looks at
static int check_mesh_shape(const char* what, const LpMeshArgs* args) {
  if (!args) return set_error(LP_ENULL, "%s: args is NULL", what);
  const LpGrid& s = args->shape;
  if (int rc = check_shape(what, "volume", s)) return rc;
  // (the product of four positive int32 can pass 2^63: compare step by step)
  int64_t n = 1;
  for (const int64_t e : {(int64_t)s.B, (int64_t)s.D, (int64_t)s.H, (int64_t)s.W}) {
    n *= e;
    if (n >= ((int64_t)1 << 31))
      return set_error(LP_EUNSUPPORTED, "%s: volume shape [%d,%d,%d,%d]: B * D * H * W has to stay below 2^31", what, s.B, s.D, s.H, s.W);
  }
  return LP_OK;
}

// everything lp_mesh_count / lp_mesh_emit check
static int check_mesh(const char* what, const LpMeshArgs* args, const void* workspace, int64_t workspace_bytes, bool emit) {
  int rc;
  if ((rc = check_mesh_shape(what, args))) return rc;
  const struct { const char* field; const void* p; } ptrs[] = {
      {"volume", args->volume},     {"vertex_offsets", args->vertex_offsets}, {"face_offsets", args->face_offsets},
      {"vertices", args->vertices}, {"faces", args->faces},                   {"normals", args->normals},
      {"workspace", workspace}};
  for (const auto& f : ptrs)
    if ((rc = check_aligned(f.field, f.p))) return rc;
  if (!args->volume) return set_error(LP_ENULL, "%s: volume is NULL", what);
  if (!args->vertex_offsets || !args->face_offsets) return set_error(LP_ENULL, "%s: vertex_offsets / face_offsets is NULL", what);
  // (its alignment was judged above, with every other pointer's)
  if ((rc = check_workspace(what, "lp_mesh_workspace_bytes", workspace, workspace_bytes, mesh_workspace_bytes(args->shape), 16, LP_ENULL))) return rc;
  if (emit) {
    if (args->max_vertices < 0 || args->max_faces < 0)
      return set_error(LP_EINVAL, "%s: max_vertices = %lld, max_faces = %lld, have to be >= 0", what, (long long)args->max_vertices,
                       (long long)args->max_faces);
    if (args->max_vertices > 0 && !args->vertices) return set_error(LP_ENULL, "%s: vertices is NULL with max_vertices = %lld", what, (long long)args->max_vertices);
    if (args->max_faces > 0 && !args->faces) return set_error(LP_ENULL, "%s: faces is NULL with max_faces = %lld", what, (long long)args->max_faces);
  }
  return LP_OK;
}

// everything lp_ray_samples_forward / _backward check.  Messages begin with the field (no entry-point prefix).
static int check_ray_samples(const LpRaySamplesArgs* args, bool backward) {
  if (!args) return set_error(LP_ENULL, "args is NULL");
  int rc;
  const LpRays& r = args->rays;
  if ((rc = check_ray_pointers(nullptr, r, false))) return rc;
  if ((rc = check_aligned("rays.encoding", r.encoding))) return rc;
  LP_ALIGNED(*args, points);
  LP_ALIGNED(*args, depths);
  LP_ALIGNED(*args, deltas);
  LP_ALIGNED(*args, grad_points);
  LP_ALIGNED(*args, grad_depths);
  LP_ALIGNED(*args, grad_deltas);
  LP_ALIGNED(*args, grad_origins);
  LP_ALIGNED(*args, grad_directions);
  LP_ALIGNED(*args, grad_near);
  LP_ALIGNED(*args, grad_far);
  if ((rc = check_march(args->march))) return rc;
  const int64_t S_tot = (int64_t)args->march.num_samples + args->march.num_samples_inf;
  if ((rc = check_point_batch(nullptr, r.n_rays, S_tot, true))) return rc;
  if (r.n_rays == 0) return LP_OK;
  // (grid_idx and encoding are not read: check_ray_pointers' rule for the marchers does not apply)
  const struct { const char* field; const void* p; bool needed; } ptrs[] = {
      {"rays.directions", r.directions, true}, {"rays.origins", r.origins, true}, {"rays.near_t", r.near_t, true},
      {"rays.far_t", r.far_t, true},           {"points", args->points, !backward}, {"depths", args->depths, !backward},
      {"deltas", args->deltas, !backward}};
  for (const auto& f : ptrs)
    if (f.needed && !f.p) return set_error(LP_ENULL, "%s is NULL", f.field);
  return LP_OK;
}

// everything lp_composite_forward / _backward check.  Messages begin with the field.
static int check_composite(const LpCompositeArgs* args, bool backward) {
  if (!args) return set_error(LP_ENULL, "args is NULL");
  int rc;
  LP_ALIGNED(*args, opacity);
  LP_ALIGNED(*args, features);
  LP_ALIGNED(*args, depths);
  LP_ALIGNED(*args, deltas);
  LP_ALIGNED(*args, ray_length);
  LP_ALIGNED(*args, neg_log_t);
  LP_ALIGNED(*args, feature);
  LP_ALIGNED(*args, weights);
  LP_ALIGNED(*args, grad_ray_length);
  LP_ALIGNED(*args, grad_neg_log_t);
  LP_ALIGNED(*args, grad_feature);
  LP_ALIGNED(*args, grad_weights);
  LP_ALIGNED(*args, grad_opacity);
  LP_ALIGNED(*args, grad_features);
  LP_ALIGNED(*args, grad_depths);
  LP_ALIGNED(*args, grad_deltas);
  if (args->n_samples < 1) return set_error(LP_EINVAL, "n_samples %d < 1", args->n_samples);
  if ((rc = check_point_batch(nullptr, args->n_rays, args->n_samples, true))) return rc;
  if (args->channels < 0 || args->channels > LP_MAX_WIDTH)
    return set_error(LP_EUNSUPPORTED, "channels %d outside [0, %d]", args->channels, LP_MAX_WIDTH);
  if (args->n_rays == 0) return LP_OK;
  const bool feat = args->channels > 0;
  const struct { const char* field; const void* p; bool needed; } ptrs[] = {
      {"opacity", args->opacity, true},          {"depths", args->depths, true},          {"deltas", args->deltas, true},
      {"ray_length", args->ray_length, !backward}, {"neg_log_t", args->neg_log_t, !backward},
      {"feature", args->feature, feat && !backward}};
  for (const auto& f : ptrs)
    if (f.needed && !f.p) return set_error(LP_ENULL, "%s is NULL", f.field);
  if (feat && !args->features) return set_error(LP_ENULL, "features is NULL with channels = %d", args->channels);
  return LP_OK;
}

// everything lp_importance_samples_forward / _backward check.  Messages begin with the field.
static int check_importance(const LpImportanceArgs* args, bool backward) {
  if (!args) return set_error(LP_ENULL, "args is NULL");
  int rc;
  LP_ALIGNED(*args, origins);
  LP_ALIGNED(*args, directions);
  LP_ALIGNED(*args, depths);
  LP_ALIGNED(*args, weights);
  LP_ALIGNED(*args, jitter);
  LP_ALIGNED(*args, out_points);
  LP_ALIGNED(*args, out_depths);
  LP_ALIGNED(*args, out_deltas);
  LP_ALIGNED(*args, grad_points);
  LP_ALIGNED(*args, grad_origins);
  LP_ALIGNED(*args, grad_directions);
  if (args->n_samples < 2) return set_error(LP_EINVAL, "n_samples %d < 2", args->n_samples);
  if (args->n_importance < 1) return set_error(LP_EINVAL, "n_importance %d < 1", args->n_importance);
  if (!std::isfinite(args->pad) || !(args->pad > 0.0f)) return set_error(LP_EINVAL, "pad %g has to be finite and > 0", (double)args->pad);
  if (args->n_samples > LP_IMPORTANCE_MAX) return set_error(LP_EUNSUPPORTED, "n_samples %d > %d", args->n_samples, LP_IMPORTANCE_MAX);
  if (args->n_importance > LP_IMPORTANCE_MAX)
    return set_error(LP_EUNSUPPORTED, "n_importance %d > %d", args->n_importance, LP_IMPORTANCE_MAX);
  // (the bound holds whatever include_coarse says: one rule for the forward and the backward of either layout)
  if ((rc = check_point_batch(nullptr, args->n_rays, (int64_t)args->n_samples + args->n_importance, true))) return rc;
  if (args->n_rays == 0) return LP_OK;
  const struct { const char* field; const void* p; bool needed; } ptrs[] = {
      {"origins", args->origins, !backward},       {"directions", args->directions, true},
      {"depths", args->depths, !backward},         {"weights", args->weights, !backward},
      {"out_points", args->out_points, !backward}, {"out_depths", args->out_depths, true},
      {"out_deltas", args->out_deltas, !backward}, {"grad_points", args->grad_points, backward}};
  for (const auto& f : ptrs)
    if (f.needed && !f.p) return set_error(LP_ENULL, "%s is NULL", f.field);
  return LP_OK;
}

// everything lp_distortion_forward / _backward check.  Messages begin with the field.
static int check_distortion(const LpDistortionArgs* args, bool backward) {
  if (!args) return set_error(LP_ENULL, "args is NULL");
  int rc;
  LP_ALIGNED(*args, weights);
  LP_ALIGNED(*args, depths);
  LP_ALIGNED(*args, deltas);
  LP_ALIGNED(*args, grad_loss);
  LP_ALIGNED(*args, loss);
  LP_ALIGNED(*args, grad_weights);
  LP_ALIGNED(*args, grad_depths);
  LP_ALIGNED(*args, grad_deltas);
  if (args->n_samples < 1) return set_error(LP_EINVAL, "n_samples %d < 1", args->n_samples);
  if (args->n_samples > LP_RAY_LOSS_MAX) return set_error(LP_EUNSUPPORTED, "n_samples %d > %d", args->n_samples, LP_RAY_LOSS_MAX);
  if ((rc = check_point_batch(nullptr, args->n_rays, args->n_samples, true))) return rc;
  if (args->n_rays == 0) return LP_OK;
  const struct { const char* field; const void* p; bool needed; } ptrs[] = {
      {"weights", args->weights, true}, {"depths", args->depths, true}, {"deltas", args->deltas, true}, {"loss", args->loss, !backward}};
  for (const auto& f : ptrs)
    if (f.needed && !f.p) return set_error(LP_ENULL, "%s is NULL", f.field);
  return LP_OK;
}

// everything lp_interlevel_forward / _backward check.  Messages begin with the field.
static int check_interlevel(const LpInterlevelArgs* args, bool backward) {
  if (!args) return set_error(LP_ENULL, "args is NULL");
  int rc;
  LP_ALIGNED(*args, weights);
  LP_ALIGNED(*args, depths);
  LP_ALIGNED(*args, proposal_weights);
  LP_ALIGNED(*args, proposal_depths);
  LP_ALIGNED(*args, grad_loss);
  LP_ALIGNED(*args, loss);
  LP_ALIGNED(*args, grad_proposal_weights);
  if (args->n_samples < 2) return set_error(LP_EINVAL, "n_samples %d < 2", args->n_samples);
  if (args->n_proposal < 2) return set_error(LP_EINVAL, "n_proposal %d < 2", args->n_proposal);
  if (!std::isfinite(args->eps) || !(args->eps > 0.0f)) return set_error(LP_EINVAL, "eps %g has to be finite and > 0", (double)args->eps);
  if (args->n_samples > LP_RAY_LOSS_MAX) return set_error(LP_EUNSUPPORTED, "n_samples %d > %d", args->n_samples, LP_RAY_LOSS_MAX);
  if (args->n_proposal > LP_RAY_LOSS_MAX) return set_error(LP_EUNSUPPORTED, "n_proposal %d > %d", args->n_proposal, LP_RAY_LOSS_MAX);
  if ((rc = check_point_batch(nullptr, args->n_rays, std::max(args->n_samples, args->n_proposal), true))) return rc;
  if (args->n_rays == 0) return LP_OK;
  const struct { const char* field; const void* p; bool needed; } ptrs[] = {
      {"weights", args->weights, true},
      {"depths", args->depths, true},
      {"proposal_weights", args->proposal_weights, true},
      {"proposal_depths", args->proposal_depths, true},
      {"loss", args->loss, !backward},
      {"grad_proposal_weights", args->grad_proposal_weights, backward}};
  for (const auto& f : ptrs)
    if (f.needed && !f.p) return set_error(LP_ENULL, "%s is NULL", f.field);
  return LP_OK;
}

// everything lp_render_samples_forward / _backward share; fills the normalised copy.  The decoder, the grid-lists and the scaffold go
// through the checks of the decoder at points (the colour head always takes part in the forward; in the backward with grad_feature).
// Messages begin with the field where a field is at fault.
static int check_render_samples(const char* what, const LpRenderSamplesArgs* args, bool backward, LpRenderSamplesArgs& a) {
  int rc;
  if (!args) return set_error(LP_ENULL, "%s: args is NULL", what);
  const bool color = backward ? args->grad_feature != nullptr : true;
  if ((rc = check_grid_list_aligned("grid", args->grid))) return rc;
  if ((rc = check_grid_list_aligned("color_grid", args->color_grid))) return rc;
  LP_ALIGNED(*args, mlp_params);
  LP_ALIGNED(*args, origins);
  LP_ALIGNED(*args, directions);
  LP_ALIGNED(*args, grid_idx);
  LP_ALIGNED(*args, encoding);
  LP_ALIGNED(*args, depths);
  LP_ALIGNED(*args, deltas);
  LP_ALIGNED(*args, scaffold);
  LP_ALIGNED(*args, ray_length);
  LP_ALIGNED(*args, neg_log_t);
  LP_ALIGNED(*args, feature);
  LP_ALIGNED(*args, weights);
  LP_ALIGNED(*args, chunk_nlt);
  LP_ALIGNED(*args, grad_ray_length);
  LP_ALIGNED(*args, grad_neg_log_t);
  LP_ALIGNED(*args, grad_feature);
  LP_ALIGNED(*args, grad_weights);
  LP_ALIGNED(*args, grad_grid);
  LP_ALIGNED(*args, grad_color_grid);
  if ((rc = check_ptr_list_aligned("grad_grid_list", args->grad_grid_list))) return rc;
  if ((rc = check_ptr_list_aligned("grad_color_grid_list", args->grad_color_grid_list))) return rc;
  LP_ALIGNED(*args, grad_mlp_params);
  LP_ALIGNED(*args, grad_encoding);
  if (args->n_samples < 1) return set_error(LP_EINVAL, "n_samples %d < 1", args->n_samples);
  if ((rc = check_point_batch(what, args->n_rays, args->n_samples, true))) return rc;
  if ((rc = check_grid_list("grid", args->grid, SAMPLED))) return rc;
  if ((rc = check_grid_list("color_grid", args->color_grid, SAMPLED_OR_ABSENT))) return rc;
  if ((rc = check_color_grid(what, args->grid, args->color_grid, args->trunk))) return rc;
  int head_in;
  if ((rc = check_trunk_and_opacity(what, args->grid.channels, args->trunk, args->opacity, head_in))) return rc;
  const int64_t n_to = mlp_numel(args->trunk) + mlp_numel(args->opacity);
  if ((rc = check_color_head(what, args->color, head_in, n_to, true, args->color_chn, args->encoding_dim))) return rc;
  if ((rc = check_param_count(what, n_to + mlp_numel(args->color), args->n_mlp_params, false))) return rc;
  if (args->scaffold && (rc = check_scaffold_for_grid(what, args->scaffold_shape, args->grid))) return rc;
  if (!args->mlp_params) return set_error(LP_ENULL, "%s: mlp_params is NULL", what);
  if (args->n_rays > 0) {  // (an empty batch has no tensors to point at)
    const struct { const char* field; const void* p; bool needed; } ptrs[] = {
        {"origins", args->origins, true}, {"directions", args->directions, true}, {"grid_idx", args->grid_idx, true},
        {"encoding", args->encoding, true}, {"depths", args->depths, true}, {"deltas", args->deltas, true},
        {"chunk_nlt", args->chunk_nlt, backward}};
    for (const auto& f : ptrs)
      if (f.needed && !f.p) return set_error(LP_ENULL, "%s is NULL", f.field);
  }
  a = *args;
  if (!normalize_grid_list(a.grid)) return set_error(LP_ENULL, "%s: grid.data is NULL (and a grid has no pointer of its own)", what);
  if (color && !normalize_grid_list(a.color_grid))
    return set_error(LP_ENULL, "%s: color_grid.data is NULL (and a grid has no pointer of its own)", what);
  if (backward) {
    if ((rc = normalize_grad_list("grad_grid", a.grad_grid_list, a.grad_grid, a.grid.n_grids))) return rc;
    if ((rc = normalize_grad_list("grad_color_grid", a.grad_color_grid_list, a.grad_color_grid, a.color_grid.n_grids))) return rc;
  }
  return LP_OK;
}

// everything the three lp_ray_grid_* entry points check; fills the normalised copy.  mode: 0 splat, 1 gather, 2 grad_samples.  Messages
// begin with the field where a field is at fault.  The NULL checks do not wait for a non-empty batch: the Python front-end never
// calls with one, and a C caller's mistake shows whatever the sizes are.
static int check_ray_grid(const char* what, const LpRayGridArgs* args, int mode, LpRayGridArgs& a) {
  int rc;
  if (!args) return set_error(LP_ENULL, "%s: args is NULL", what);
  if ((rc = check_grid_list_aligned("grid", args->grid))) return rc;
  if ((rc = check_ptr_list_aligned("row_weight", args->row_weight))) return rc;
  LP_ALIGNED(*args, origins);
  LP_ALIGNED(*args, directions);
  LP_ALIGNED(*args, grid_idx);
  LP_ALIGNED(*args, depths);
  LP_ALIGNED(*args, weights);
  LP_ALIGNED(*args, vectors);
  LP_ALIGNED(*args, out_features);
  LP_ALIGNED(*args, grad_weights);
  LP_ALIGNED(*args, grad_depths);
  if (args->n_rays < 0) return set_error(LP_EINVAL, "n_rays %lld < 0", (long long)args->n_rays);
  if (args->n_samples < 0) return set_error(LP_EINVAL, "n_samples %d < 0", args->n_samples);
  if ((rc = check_point_batch(what, args->n_rays, args->n_samples, true))) return rc;
  if ((rc = check_grid_list("grid", args->grid, SAMPLED))) return rc;
  if (args->channels != args->grid.channels)
    return set_error(LP_EINVAL, "channels %d of the per-ray vectors != grid channels %d", args->channels, args->grid.channels);
  int have = 0;
  for (int g = 0; g < args->grid.n_grids; ++g) have += args->row_weight[g] != nullptr;
  if (mode == 0 && have != 0 && have != args->grid.n_grids)
    return set_error(LP_EINVAL, "row_weight given for %d of %d grids (all or none)", have, args->grid.n_grids);
  const struct { const char* field; const void* p; bool needed; } ptrs[] = {
      {"origins", args->origins, true},   {"directions", args->directions, true},  {"grid_idx", args->grid_idx, true},
      {"depths", args->depths, true},     {"weights", args->weights, true},        {"vectors", args->vectors, mode != 1},
      {"out_features", args->out_features, mode == 1}};
  for (const auto& f : ptrs)
    if (f.needed && !f.p) return set_error(LP_ENULL, "%s is NULL", f.field);
  if (mode == 2 && !args->grad_weights && !args->grad_depths)
    return set_error(LP_ENULL, "grad_weights and grad_depths are both NULL: %s has no result to write", what);
  a = *args;
  if (!normalize_grid_list(a.grid)) return set_error(LP_ENULL, "%s: grid.data is NULL (and a grid has no pointer of its own)", what);
  for (int g = a.grid.n_grids; g < LP_MAX_GRIDS; ++g) a.row_weight[g] = nullptr;
  return LP_OK;
}

// the "points" entry of lp_build_info() also reports the render at given depths (lp_render_samples.hip is the decoder at points fused
// with the compositing): the top-level keys of the text stay as they are
static const char* build_info_points_family() {
  static char text[2048];
  const char* p = build_info_points();
  snprintf(text, sizeof(text), "%.*s, \"render_samples\": %s}", (int)strlen(p) - 1, p, build_info_render_samples());
  return text;
}

}  // namespace lp

using namespace lp;

extern "C" {

int lp_version(void) { return LP_VERSION; }

const char* lp_last_error(void) { return g_err; }

const char* lp_build_info(void) {
  static char info[8192];
  // what every translation unit reports about itself (a JSON fragment each), in the order of the text
  static const struct { const char* key; const char* (*value)(); } units[] = {
      {"test_hooks", build_info_tuned_bwd_aux}, {"tuned_bwd", build_info_tuned_bwd},          {"loop_bwd_deep", build_info_loop_deep},
      {"loop_bwd_shallow", build_info_loop_shallow}, {"mlp_splatter_bwd", build_info_splatter_mlp}, {"loop_fwd_stream", build_info_loop_stream},
      {"grid_tv", build_info_grid_tv},          {"grid_resample", build_info_grid_resample},  {"scaffold", build_info_scaffold},
      {"points", build_info_points_family},     {"ray_clip", build_info_ray_clip},           {"point_grid", build_info_point_grid},
      {"mesh", build_info_mesh}};
  static const bool once = [] {
    size_t n = (size_t)snprintf(info, sizeof(info), "{\"version\": %d, \"src_hash\": \"%s\"", lp_version(), LP_BUILD_SRC_HASH);
    for (const auto& u : units)
      if (n < sizeof(info)) n += (size_t)snprintf(info + n, sizeof(info) - n, ", \"%s\": %s", u.key, u.value());
    if (n < sizeof(info))
      snprintf(info + n, sizeof(info) - n,
               ", \"forward\": \"bf16x3 (three exact bf16 limbs per fp32 operand, six limb products, fp32 accumulation) on "
               "v_mfma_f32_32x32x16_bf16; generic kernels: fp32 FMA\", \"flags\": %s}",
               LP_BUILD_FLAGS_JSON);
    return true;
  }();
  (void)once;
  return info;
}

int lp_abi_sizeof(int which) {
  switch (which) {
    case 0: return (int)sizeof(LpGrid);
    case 1: return (int)sizeof(LpGridList);
    case 2: return (int)sizeof(LpRays);
    case 3: return (int)sizeof(LpMarch);
    case 4: return (int)sizeof(LpMlp);
    case 5: return (int)sizeof(LpRendererArgs);
    case 6: return (int)sizeof(LpSplatterArgs);
    case 7: return (int)sizeof(LpRayEmbedArgs);
    case 8: return (int)sizeof(LpScaffoldArgs);
    case 10: return (int)sizeof(LpPointsArgs);  // (9 stays unanswered: lightplane_hip.h)
    case 12: return (int)sizeof(LpRayClipArgs);  // (and so does 11)
    case 14: return (int)sizeof(LpPointGridArgs);  // (and 13)
    case 16: return (int)sizeof(LpMeshArgs);  // (and 15)
    case 18: return (int)sizeof(LpRaySamplesArgs);  // (and 17; this one and the next: lightplane_hip_samples.h)
    case 20: return (int)sizeof(LpCompositeArgs);  // (and 19)
    case 22: return (int)sizeof(LpImportanceArgs);  // (and 21: lightplane_hip_importance.h)
    case 24: return (int)sizeof(LpDistortionArgs);  // (and 23; this one and the next: lightplane_hip_losses.h)
    case 26: return (int)sizeof(LpInterlevelArgs);  // (and 25)
    case 30: return (int)sizeof(LpRenderSamplesArgs);  // (and 27, 28, 29: lightplane_hip_render_samples.h)
    case 34: return (int)sizeof(LpRayGridArgs);  // (and 31, 32, 33: lightplane_hip_ray_grid.h)
    default: return -1;
  }
}

// kernel selection: 1 = the tuned bf16x3 kernels of the default shape (2/2/2 x 32), 3 = layer-looped bf16x3 MFMA family (1-4 layers
// per MLP, widths 16 / 32 / 64), 0 = the shape-generic kernel.  (2 was the fp32-MFMA family of 2/2/2 x 64, retired in 0.2.4: the
// two-block looped kernels with the eight-wave forward measure 1-2 % faster forward + backward and 25-29 % faster forward on it --
// profiles/r04_h64_looped_vs_wide.txt.)  LP_LOOP=1 (developer knob, read once): the layer-looped family also for the shape family 1
// covers (A/B, test coverage).
// LP_ARITH_FP32 (LpRendererArgs.arithmetic): the tuned family where it has such instantiations, the generic fp32 kernels otherwise.
static int select_renderer(const LpRendererArgs& a, const char** why) {
  const char* w32 = "";
  const char* wl = "";
  if (a.arithmetic == LP_ARITH_FP32) {
    if (renderer_mfma_f32_supported(a)) return 1;
    *why = "LP_ARITH_FP32 outside the tuned family's four-wave instantiations: shape-generic fp32 kernels";
    return 0;
  }
  static const bool force_loop = getenv("LP_LOOP") != nullptr && atoi(getenv("LP_LOOP")) != 0;
  const bool loop_ok = renderer_loop_supported(a, &wl) && renderer_loop_fits(a);
  if (force_loop && loop_ok) return 3;
  if (renderer_mfma_supported(a, &w32)) return 1;
  if (loop_ok) return 3;
  *why = wl[0] ? wl : "weight images of this decoder exceed the 160 KB LDS";
  return 0;
}

int lp_renderer_kernel_family(const LpRendererArgs* args) {
  if (!args) return set_error(LP_ENULL, "args is NULL");
  const char* why = "";
  return select_renderer(*args, &why);
}

int lp_renderer_backward_segments(const LpRendererArgs* args) {
  if (!args) return set_error(LP_ENULL, "args is NULL");
  const char* why = "";
  if (args->kernel == LP_KERNEL_GENERIC) return 1;
  const int fam = select_renderer(*args, &why);
  return fam == 1 ? renderer_mfma_segments(*args) : fam == 3 ? renderer_loop_segments(*args) : 1;
}

// MLP-Splatter: 3 = layer-looped bf16x3 family (2-4 layers, widths 16 / 32 / 64), 0 = generic.  (2 was the two-layer fp32-MFMA
// family [E,32,Cout] of rounds 1-3, retired in round 4: the looped family's two-waves-per-SIMD backward measures within 1 % of
// it or faster on every shape it covered -- profiles/r04_loop_shallow_ab.txt.)
static int splatter_mlp_family(const LpSplatterArgs& a) { return splatter_mlp_loop_supported(a) ? 3 : 0; }

int lp_splatter_kernel_family(const LpSplatterArgs* args) {
  if (!args) return set_error(LP_ENULL, "args is NULL");
  if (args->mlp.n_layers > 0) return splatter_mlp_family(*args);
  const int C = args->out.channels;
  return ((C == 16 || C == 32 || C == 64) && args->out.n_rows < ((int64_t)1 << 31)) ? 1 : 0;
}

// copy of the caller's arguments with every per-grid pointer made explicit (what the kernels read)
static int normalized_renderer_args(const LpRendererArgs* args, bool backward, LpRendererArgs& a) {
  int rc = check_renderer(*args, backward);
  if (rc) return rc;
  a = *args;
  const bool have_grid = normalize_grid_list(a.grid);
  const bool have_cgrid = normalize_grid_list(a.color_grid);
  if (a.rays.n_rays > 0 && !have_grid) return set_error(LP_ENULL, "grid.data is NULL (and a grid has no pointer of its own)");
  if (a.rays.n_rays > 0 && !have_cgrid) return set_error(LP_ENULL, "color_grid.data is NULL (and a grid has no pointer of its own)");
  if ((rc = normalize_grad_list("grad_grid", a.grad_grid_list, backward ? a.grad_grid : nullptr, a.grid.n_grids))) return rc;
  if ((rc = normalize_grad_list("grad_color_grid", a.grad_color_grid_list, backward ? a.grad_color_grid : nullptr,
                                a.color_grid.n_grids)))
    return rc;
  if (a.alpha_mode < 0 || a.alpha_mode > 2) return set_error(LP_EINVAL, "alpha_mode %d outside 0..2", a.alpha_mode);
  if ((a.alpha || a.grad_alpha) && a.alpha_mode == 0)
    return set_error(LP_EINVAL, "alpha / grad_alpha given but alpha_mode is 0");
  // the segment sums are written / used only where lp_renderer_backward_segments() says so (same rule both ways)
  if (a.seg_prefix && lp_renderer_backward_segments(&a) <= 1) a.seg_prefix = nullptr;
  return LP_OK;
}

// checks and normalises, picks the family (LP_KERNEL_MFMA refuses the shape-generic one) and launches its forward or backward
static int renderer_dispatch(const LpRendererArgs* args, bool backward, hipStream_t stream) {
  if (!args) return set_error(LP_ENULL, "args is NULL");
  LpRendererArgs a;
  const int rc = normalized_renderer_args(args, backward, a);
  if (rc) return rc;
  const char* why = "";
  int fam = select_renderer(a, &why);
  if (a.kernel == LP_KERNEL_MFMA && fam == 0)
    return set_error(LP_EUNSUPPORTED, "MFMA renderer kernel unavailable for this shape: %s", why);
  if (a.kernel == LP_KERNEL_GENERIC) fam = 0;
  if (fam == 1) return backward ? renderer_backward_mfma(a, stream) : renderer_forward_mfma(a, stream);
  if (backward) g_last_backward = fam == 3 ? "layer-looped family" : "shape-generic kernels";  // (the tuned family names its own march)
  if (fam == 3) return backward ? renderer_backward_loop(a, stream) : renderer_forward_loop(a, stream);
  return backward ? renderer_backward_generic(a, stream) : renderer_forward_generic(a, stream);
}

int lp_renderer_forward(const LpRendererArgs* args, void* stream) { return renderer_dispatch(args, false, (hipStream_t)stream); }

// The forward's own selection (lp_renderer_forward_ws): the family of lp_renderer_kernel_family, and on the shapes that one turns down
// only for their depth at hidden width 64 / 64 grid channels the layer-looped forward -- 3 with resident weight images, 4 streamed.
static bool deep_forward(const LpRendererArgs& a, int fam) {
  return fam == 0 && a.kernel != LP_KERNEL_GENERIC && renderer_deep_forward_supported(a);
}

int lp_renderer_forward_family(const LpRendererArgs* args) {
  if (!args) return set_error(LP_ENULL, "args is NULL");
  if (args->kernel == LP_KERNEL_GENERIC) return 0;
  const char* why = "";
  const int fam = select_renderer(*args, &why);
  return deep_forward(*args, fam) ? renderer_deep_forward_family(*args) : fam;
}

int64_t lp_renderer_forward_workspace_bytes(const LpRendererArgs* args) {
  if (!args) return set_error(LP_ENULL, "args is NULL");
  const char* why = "";
  return deep_forward(*args, select_renderer(*args, &why)) ? renderer_deep_forward_workspace(*args) : 0;
}

int lp_renderer_forward_ws(const LpRendererArgs* args, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!args) return set_error(LP_ENULL, "args is NULL");
  LpRendererArgs a;
  int rc = normalized_renderer_args(args, false, a);
  if (rc) return rc;
  const char* why = "";
  if (deep_forward(a, select_renderer(a, &why))) return renderer_forward_deep(a, workspace, workspace_bytes, (hipStream_t)stream);
  return lp_renderer_forward(args, stream);
}

int lp_renderer_backward(const LpRendererArgs* args, void* stream) { return renderer_dispatch(args, true, (hipStream_t)stream); }

int lp_renderer_corner_rows(const LpRendererArgs* args, int64_t* rows, void* stream) {
  if (!args || !rows) return set_error(LP_ENULL, "args / rows is NULL");
  int rc;
  if ((rc = check_rays(args->rays, false))) return rc;
  if ((rc = check_march(args->march))) return rc;
  if ((rc = check_grid_list("grid", args->grid, SAMPLED))) return rc;
  return renderer_corner_rows_launch(*args, rows, (hipStream_t)stream);
}

int lp_renderer_relu_dump_words(const LpRendererArgs* args) {
  if (!args) return set_error(LP_ENULL, "args is NULL");
  const char* why = "";
  const int fam = args->kernel == LP_KERNEL_GENERIC ? 0 : select_renderer(*args, &why);
  if (args->arithmetic != LP_ARITH_DEFAULT) return set_error(LP_EUNSUPPORTED, "relu dump: the LP_ARITH_FP32 instantiations have no dump twin");
  if (fam == 1) {
    if (args->march.num_samples_inf > 64) return set_error(LP_EUNSUPPORTED, "relu dump: the tuned family's eight-wave workgroups (> 64 beyond-far samples) have no dump twin");
    return 5;
  }
  if (fam == 3) return renderer_loop_dump_words(*args);
  return renderer_generic_dump_words(*args);  // (the shape-generic backward: ceil(widest site / 32) words per site)
}

int lp_renderer_backward_relu_dump(const LpRendererArgs* args, uint32_t* dump, int64_t dump_words, void* stream) {
  if (!args || !dump) return set_error(LP_ENULL, "args / dump is NULL");
  LpRendererArgs a;
  int rc = normalized_renderer_args(args, true, a);
  if (rc) return rc;
  const int w = lp_renderer_relu_dump_words(&a);
  if (w < 0) return w;
  if ((rc = check_dump_words(args->rays, args->march, w, dump_words))) return rc;
  g_relu_dump = dump;
  rc = lp_renderer_backward(args, stream);
  g_relu_dump = nullptr;
  return rc;
}

static int normalized_splatter_args(const LpSplatterArgs* args, bool backward, LpSplatterArgs& a) {
  int rc = check_splatter(*args, backward);
  if (rc) return rc;
  a = *args;
  if (a.mlp.n_layers > 0) {
    if (!normalize_grid_list(a.input_grid) && a.rays.n_rays > 0)
      return set_error(LP_ENULL, "input_grid.data is NULL (and a grid has no pointer of its own)");
    if ((rc = normalize_grad_list("grad_input_grid", a.grad_input_grid_list, backward ? a.grad_input_grid : nullptr,
                                  a.input_grid.n_grids)))
      return rc;
  }
  return LP_OK;
}

// checks and normalises and launches the forward or backward: of the plain Splatter, or of the MLP-Splatter's family (LP_KERNEL_MFMA
// refuses the shape-generic one)
static int splatter_dispatch(const LpSplatterArgs* args, bool backward, hipStream_t stream) {
  if (!args) return set_error(LP_ENULL, "args is NULL");
  LpSplatterArgs a;
  const int rc = normalized_splatter_args(args, backward, a);
  if (rc) return rc;
  if (a.mlp.n_layers == 0) return backward ? splatter_backward_launch(a, stream) : splatter_forward_launch(a, stream);
  const int fam = splatter_mlp_family(a);
  if (a.kernel == LP_KERNEL_MFMA && fam == 0) return set_error(LP_EUNSUPPORTED, "MFMA MLP-splatter kernel unavailable for this shape");
  if (fam == 3 && a.kernel != LP_KERNEL_GENERIC) return backward ? splatter_mlp_backward_loop(a, stream) : splatter_mlp_forward_loop(a, stream);
  return backward ? splatter_mlp_backward_launch(a, stream) : splatter_mlp_forward_launch(a, stream);
}

int lp_splatter_forward(const LpSplatterArgs* args, void* stream) { return splatter_dispatch(args, false, (hipStream_t)stream); }

int lp_splatter_normalize(float* feature, const float* weight, int64_t n_rows, int32_t channels, void* stream) {
  if (n_rows < 0 || channels < 1) return set_error(LP_EINVAL, "normalize: bad shape [%lld, %d]", (long long)n_rows, channels);
  int rc;
  if ((rc = check_aligned("feature", feature)) || (rc = check_aligned("weight", weight))) return rc;
  if (n_rows > 0 && (!feature || !weight)) return set_error(LP_ENULL, "normalize: NULL buffer");
  return splatter_normalize_launch(feature, weight, n_rows, channels, (hipStream_t)stream);
}

int lp_splatter_backward(const LpSplatterArgs* args, void* stream) { return splatter_dispatch(args, true, (hipStream_t)stream); }

int lp_mlp_splatter_relu_dump_words(const LpSplatterArgs* args) {
  if (!args) return set_error(LP_ENULL, "args is NULL");
  int rc;
  if ((rc = check_mlp("splatter", args->mlp, false))) return rc;
  if (args->mlp.n_layers < 2) return set_error(LP_EINVAL, "relu dump: a one-layer MLP has no ReLU");
  if (args->kernel != LP_KERNEL_GENERIC && splatter_mlp_family(*args) == 3) return splatter_mlp_loop_dump_words(*args);
  return splatter_mlp_dump_words(*args);
}

int lp_mlp_splatter_backward_relu_dump(const LpSplatterArgs* args, uint32_t* dump, int64_t dump_words, void* stream) {
  if (!args || !dump) return set_error(LP_ENULL, "args / dump is NULL");
  const int w = lp_mlp_splatter_relu_dump_words(args);
  if (w < 0) return w;
  if (int rc = check_dump_words(args->rays, args->march, w, dump_words)) return rc;
  g_relu_dump = dump;
  const int rc = lp_splatter_backward(args, stream);
  g_relu_dump = nullptr;
  return rc;
}

int lp_mlp_splatter_launch_shape(const LpSplatterArgs* args, int32_t* shape) {
  if (!args || !shape) return set_error(LP_ENULL, "args / shape is NULL");
  int rc;
  if ((rc = check_mlp("splatter", args->mlp, false))) return rc;
  const int fam = args->kernel == LP_KERNEL_GENERIC ? 0 : splatter_mlp_family(*args);
  if (args->kernel == LP_KERNEL_MFMA && fam == 0) return set_error(LP_EUNSUPPORTED, "MFMA MLP-splatter kernel unavailable for this shape");
  shape[0] = fam;
  if (fam == 3) {
    splatter_mlp_loop_shape(*args, shape);
  } else {  // one-wave workgroups, one sweep per ray both ways
    shape[1] = 1;
    shape[2] = 1;
    shape[3] = 0;
    shape[4] = 0;
    shape[5] = 1;
  }
  return LP_OK;
}

/* developer / test hook (not part of include/lightplane_hip.h): which Renderer backward the process launched last --
 * "tuned family, rays per wavefront", "tuned family, samples per wavefront (transposed march)", "layer-looped family",
 * "shape-generic kernels" (static strings) */
const char* lp_debug_last_renderer_backward(void) { return g_last_backward; }

static int check_ray_embed(const LpRayEmbedArgs& a, bool backward) {
  if (a.n_rays < 0) return set_error(LP_EINVAL, "n_rays %lld < 0", (long long)a.n_rays);
  if (a.n_harmonics < 0 || a.n_harmonics > 10) return set_error(LP_EUNSUPPORTED, "n_harmonics %d outside [0, 10]", a.n_harmonics);
  if (a.out_dim < 1 || a.out_dim > LP_MAX_WIDTH) return set_error(LP_EUNSUPPORTED, "out_dim %d outside [1, %d]", a.out_dim, LP_MAX_WIDTH);
  LP_ALIGNED(a, directions);
  LP_ALIGNED(a, weight);
  LP_ALIGNED(a, bias);
  LP_ALIGNED(a, out);
  LP_ALIGNED(a, grad_out);
  LP_ALIGNED(a, grad_weight);
  LP_ALIGNED(a, grad_bias);
  if (a.n_rays == 0) return LP_OK;
  if (!a.directions) return set_error(LP_ENULL, "directions is NULL");
  if (!backward && (!a.weight || !a.bias || !a.out)) return set_error(LP_ENULL, "weight / bias / out must be non-NULL");
  if (backward && (!a.grad_out || (!a.grad_weight && !a.grad_bias)))
    return set_error(LP_ENULL, "grad_out and at least one of grad_weight / grad_bias must be non-NULL");
  return LP_OK;
}

int lp_ray_embedding_forward(const LpRayEmbedArgs* args, void* stream) {
  if (!args) return set_error(LP_ENULL, "args is NULL");
  const int rc = check_ray_embed(*args, false);
  if (rc) return rc;
  return ray_embedding_forward_launch(*args, (hipStream_t)stream);
}

int lp_ray_embedding_backward(const LpRayEmbedArgs* args, void* stream) {
  if (!args) return set_error(LP_ENULL, "args is NULL");
  const int rc = check_ray_embed(*args, true);
  if (rc) return rc;
  return ray_embedding_backward_launch(*args, (hipStream_t)stream);
}

int lp_hash_randn(const int32_t* x1, const int32_t* x2, float* out, int64_t n, int32_t seed, void* stream) {
  if (n < 0) return set_error(LP_EINVAL, "n < 0");
  if (n > 0 && (!x1 || !x2 || !out)) return set_error(LP_ENULL, "hash_randn: NULL buffer");
  return hash_randn_launch(x1, x2, out, n, seed, (hipStream_t)stream);
}

int64_t lp_grid_tv_workspace_bytes(const LpGridList* grid) {
  const int rc = check_tv_grid_list(grid);
  if (rc) return rc;
  return grid_tv_workspace_bytes(*grid);
}

int lp_grid_tv_forward(const LpGridList* grid, const float* grid_weights, int32_t n_weights, int32_t p, float* loss, void* workspace,
                       int64_t workspace_bytes, void* stream) {
  LpGridList gl;
  const int rc = check_grid_tv("lp_grid_tv_forward", grid, grid_weights, n_weights, p, true, loss, workspace, workspace_bytes, false,
                               nullptr, nullptr, 0, gl, nullptr);
  if (rc) return rc;
  return grid_tv_launch(gl, grid_weights, p, loss, (double*)workspace, nullptr, 1.0f, nullptr, false, (hipStream_t)stream);
}

int lp_grid_tv_backward(const LpGridList* grid, const float* grid_weights, int32_t n_weights, int32_t p, const float* grad_loss,
                        float scale, float* grad, float* const* grad_list, int32_t n_grad_list, int32_t accumulate, void* stream) {
  LpGridList gl;
  float* grads[LP_MAX_GRIDS];
  const int rc = check_grid_tv("lp_grid_tv_backward", grid, grid_weights, n_weights, p, false, nullptr, nullptr, 0, true, grad,
                               grad_list, n_grad_list, gl, grads);
  if (rc) return rc;
  return grid_tv_launch(gl, grid_weights, p, nullptr, nullptr, grad_loss, scale, grads, accumulate != 0, (hipStream_t)stream);
}

int lp_grid_tv_fused(const LpGridList* grid, const float* grid_weights, int32_t n_weights, int32_t p, float* loss, void* workspace,
                     int64_t workspace_bytes, const float* grad_loss, float scale, float* grad, float* const* grad_list,
                     int32_t n_grad_list, void* stream) {
  LpGridList gl;
  float* grads[LP_MAX_GRIDS];
  const int rc = check_grid_tv("lp_grid_tv_fused", grid, grid_weights, n_weights, p, true, loss, workspace, workspace_bytes, true, grad,
                               grad_list, n_grad_list, gl, grads);
  if (rc) return rc;
  return grid_tv_launch(gl, grid_weights, p, loss, (double*)workspace, grad_loss, scale, grads, true, (hipStream_t)stream);
}

int lp_grid_resample_forward(const LpGridList* src, const LpGridList* dst, int32_t align_corners, const float* coeffs, void* stream) {
  LpGridList s, d;
  const int rc = check_grid_resample("lp_grid_resample_forward", src, dst, align_corners, coeffs, s, d);
  if (rc) return rc;
  return grid_resample_launch(s, d, align_corners, coeffs, false, false, (hipStream_t)stream);
}

int lp_grid_resample_backward(const LpGridList* grad_src, const LpGridList* grad_dst, int32_t align_corners, const float* coeffs,
                              int32_t accumulate, void* stream) {
  LpGridList s, d;
  const int rc = check_grid_resample("lp_grid_resample_backward", grad_src, grad_dst, align_corners, coeffs, s, d);
  if (rc) return rc;
  return grid_resample_launch(s, d, align_corners, coeffs, true, accumulate != 0, (hipStream_t)stream);
}

int lp_points_forward(const LpPointsArgs* args, void* stream) {
  LpPointsArgs a;
  const int rc = check_points("lp_points_forward", args, false, a);
  if (rc) return rc;
  return points_forward_launch(a, (hipStream_t)stream);
}

int lp_points_backward(const LpPointsArgs* args, void* stream) {
  LpPointsArgs a;
  const int rc = check_points("lp_points_backward", args, true, a);
  if (rc) return rc;
  return points_backward_launch(a, (hipStream_t)stream);
}

int lp_point_gather(const LpPointGridArgs* args, void* stream) {
  LpPointGridArgs a;
  const int rc = check_point_grid("lp_point_gather", args, 0, a);
  if (rc != LP_OK) return rc;
  return point_gather_launch(a, (hipStream_t)stream);
}

int lp_point_splat(const LpPointGridArgs* args, void* stream) {
  LpPointGridArgs a;
  const int rc = check_point_grid("lp_point_splat", args, 1, a);
  if (rc != LP_OK) return rc;
  return point_splat_launch(a, (hipStream_t)stream);
}

int lp_point_normalize(const LpPointGridArgs* args, void* stream) {
  LpPointGridArgs a;
  const int rc = check_point_grid("lp_point_normalize", args, 2, a);
  if (rc != LP_OK) return rc;
  return point_normalize_launch(a, (hipStream_t)stream);
}

int lp_point_grad_points(const LpPointGridArgs* args, void* stream) {
  LpPointGridArgs a;
  const int rc = check_point_grid("lp_point_grad_points", args, 3, a);
  if (rc != LP_OK) return rc;
  return point_grad_points_launch(a, (hipStream_t)stream);
}

int lp_ray_samples_forward(const LpRaySamplesArgs* args, void* stream) {
  const int rc = check_ray_samples(args, false);
  if (rc || args->rays.n_rays == 0) return rc;
  return ray_samples_launch(*args, false, (hipStream_t)stream);
}

int lp_ray_samples_backward(const LpRaySamplesArgs* args, void* stream) {
  const int rc = check_ray_samples(args, true);
  if (rc || args->rays.n_rays == 0) return rc;
  return ray_samples_launch(*args, true, (hipStream_t)stream);
}

int lp_composite_forward(const LpCompositeArgs* args, void* stream) {
  const int rc = check_composite(args, false);
  if (rc || args->n_rays == 0) return rc;
  return composite_launch(*args, false, (hipStream_t)stream);
}

int lp_composite_backward(const LpCompositeArgs* args, void* stream) {
  const int rc = check_composite(args, true);
  if (rc || args->n_rays == 0) return rc;
  return composite_launch(*args, true, (hipStream_t)stream);
}

int lp_importance_samples_forward(const LpImportanceArgs* args, void* stream) {
  const int rc = check_importance(args, false);
  if (rc || args->n_rays == 0) return rc;
  return importance_launch(*args, false, (hipStream_t)stream);
}

int lp_render_samples_chunks(int32_t n_samples) { return n_samples < 1 ? 0 : (int)(((int64_t)n_samples + 63) / 64); }

int lp_render_samples_forward(const LpRenderSamplesArgs* args, void* stream) {
  LpRenderSamplesArgs a;
  const int rc = check_render_samples("lp_render_samples_forward", args, false, a);
  if (rc != LP_OK || a.n_rays == 0) return rc;
  return render_samples_launch(a, false, (hipStream_t)stream);
}

int lp_render_samples_backward(const LpRenderSamplesArgs* args, void* stream) {
  LpRenderSamplesArgs a;
  const int rc = check_render_samples("lp_render_samples_backward", args, true, a);
  if (rc != LP_OK || a.n_rays == 0) return rc;
  return render_samples_launch(a, true, (hipStream_t)stream);
}

int lp_ray_grid_splat(const LpRayGridArgs* args, void* stream) {
  LpRayGridArgs a;
  const int rc = check_ray_grid("lp_ray_grid_splat", args, 0, a);
  if (rc != LP_OK || a.n_rays == 0 || a.n_samples == 0) return rc;
  return ray_grid_splat_launch(a, (hipStream_t)stream);
}

int lp_ray_grid_gather(const LpRayGridArgs* args, void* stream) {
  LpRayGridArgs a;
  const int rc = check_ray_grid("lp_ray_grid_gather", args, 1, a);
  if (rc != LP_OK || a.n_rays == 0 || a.n_samples == 0) return rc;
  return ray_grid_gather_launch(a, (hipStream_t)stream);
}

int lp_ray_grid_grad_samples(const LpRayGridArgs* args, void* stream) {
  LpRayGridArgs a;
  const int rc = check_ray_grid("lp_ray_grid_grad_samples", args, 2, a);
  if (rc != LP_OK || a.n_rays == 0 || a.n_samples == 0) return rc;
  return ray_grid_grad_samples_launch(a, (hipStream_t)stream);
}

int lp_importance_samples_backward(const LpImportanceArgs* args, void* stream) {
  const int rc = check_importance(args, true);
  if (rc || args->n_rays == 0) return rc;
  return importance_launch(*args, true, (hipStream_t)stream);
}

int lp_distortion_forward(const LpDistortionArgs* args, void* stream) {
  const int rc = check_distortion(args, false);
  if (rc || args->n_rays == 0) return rc;
  return distortion_launch(*args, false, (hipStream_t)stream);
}

int lp_distortion_backward(const LpDistortionArgs* args, void* stream) {
  const int rc = check_distortion(args, true);
  if (rc || args->n_rays == 0) return rc;
  return distortion_launch(*args, true, (hipStream_t)stream);
}

int lp_interlevel_forward(const LpInterlevelArgs* args, void* stream) {
  const int rc = check_interlevel(args, false);
  if (rc || args->n_rays == 0) return rc;
  return interlevel_launch(*args, false, (hipStream_t)stream);
}

int lp_interlevel_backward(const LpInterlevelArgs* args, void* stream) {
  const int rc = check_interlevel(args, true);
  if (rc || args->n_rays == 0) return rc;
  return interlevel_launch(*args, true, (hipStream_t)stream);
}

int lp_rays_clip(const LpRayClipArgs* args, float* near_out, float* far_out, uint8_t* hit_out, void* stream) {
  const int rc = check_ray_clip(args, near_out, far_out, hit_out);
  if (rc) return rc;
  if (args->rays.n_rays == 0) return LP_OK;
  return rays_clip_launch(*args, near_out, far_out, hit_out, (hipStream_t)stream);
}

int64_t lp_scaffold_workspace_bytes(const LpScaffoldArgs* args) {
  const int rc = check_scaffold_shape("lp_scaffold_workspace_bytes", args);
  if (rc) return rc;
  return scaffold_workspace_bytes(args->shape, args->dilate);
}

int lp_scaffold_opacity(const LpScaffoldArgs* args, float* opacity, void* stream) {
  LpScaffoldArgs a;
  const int rc = check_scaffold("lp_scaffold_opacity", args, opacity, a);
  if (rc) return rc;
  return scaffold_launch(a, opacity, nullptr, false, (hipStream_t)stream);
}

int lp_scaffold_build(const LpScaffoldArgs* args, float* scaffold, void* workspace, int64_t workspace_bytes, void* stream) {
  LpScaffoldArgs a;
  int rc = check_scaffold("lp_scaffold_build", args, scaffold, a);
  if (rc) return rc;
  const int64_t need = scaffold_workspace_bytes(a.shape, a.dilate);
  if (need > 0) {
    if ((rc = check_workspace("lp_scaffold_build", "lp_scaffold_workspace_bytes", workspace, workspace_bytes, need, 16, LP_EINVAL))) return rc;
    const uintptr_t w0 = (uintptr_t)workspace, s0 = (uintptr_t)scaffold;
    if (w0 < s0 + (uintptr_t)need * 4 && s0 < w0 + (uintptr_t)need)
      return set_error(LP_EINVAL, "lp_scaffold_build: the workspace overlaps the result");
  }
  return scaffold_launch(a, scaffold, workspace, true, (hipStream_t)stream);
}

int64_t lp_mesh_workspace_bytes(const LpMeshArgs* args) {
  const int rc = check_mesh_shape("lp_mesh_workspace_bytes", args);
  if (rc) return rc;
  return mesh_workspace_bytes(args->shape);
}

int lp_mesh_count(const LpMeshArgs* args, void* workspace, int64_t workspace_bytes, void* stream) {
  const int rc = check_mesh("lp_mesh_count", args, workspace, workspace_bytes, false);
  if (rc) return rc;
  return mesh_count_launch(*args, workspace, (hipStream_t)stream);
}

int lp_mesh_emit(const LpMeshArgs* args, void* workspace, int64_t workspace_bytes, void* stream) {
  const int rc = check_mesh("lp_mesh_emit", args, workspace, workspace_bytes, true);
  if (rc) return rc;
  return mesh_emit_launch(*args, workspace, (hipStream_t)stream);
}

}  // extern "C"

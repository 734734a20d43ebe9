// lp_hash_points.hip -- the decoder on a multiresolution hash grid at 3-D points, encoding and decoder in one launch (C ABI
// lp_hash_points_forward / lp_hash_points_backward, include/lightplane_hip_hash_points.h, which holds the definition).  The features
// [n_rays, n_pts, L F] of the chain hash_grid_encode -> decoder never reach memory, and neither does their gradient.
//
// Forward, hash_points_fwd<OPACITY_ONLY>: one lane = one point, one wave = one workgroup = 64 consecutive points, so a ray boundary may
// fall anywhere inside a wave.  The point's geometry (batch element, contraction, mask, scaffold) is formed once; then the lane loops
// over the LEVELS -- point-major, where the stand-alone encoding (lp_hash_grid.hip) launches level-major: a wave touches all L level
// tables -- with the level's constants read through a wave-uniform index, the 8 corner loads issued before the first use (hg_interp,
// lp_hash_levels.h) and the F results written to rows l F .. of the first LDS column tile [maxw][64].  F is dispatched by a
// wave-uniform switch around the templated level function: two instantiations of the kernel, not eight.  The rest is points_fwd
// (lp_points.hip): trunk -> opacity head ping-ponging through two tiles, a third one for the colour head's input, sc_dense with
// scalar-loaded weights.  No private array, no scratch, no atomics: bit-reproducible.
//
// Backward, hash_points_bwd<ACT_CAP, LDS_ACC>: points_bwd with the hash table in place of the grid-list.  A workgroup (one wave) takes
// a run of consecutive 64-point tiles; per tile it recomputes the features into act[x0 ..] (the same level function) and the decoder
// behind them (decode_gathered, lp_generic_decode.h), forms d raw / d craw, runs mlp_backward through the colour head, the opacity head
// and the trunk (weight gradients into LDS accumulators flushed once per workgroup) and encoding_grad_wave.  Then ONE loop over the
// levels with the lane's d feat[l F ..]: the table gradient leaves as run-merged fp32 atomics (hg_run / hg_table_grad: lanes are
// consecutive points, so consecutive samples of a ray form runs on the coarse levels) and the point gradient gathers
// sum_k (d w_k / d x) <table row, d feat_l> N_l / 2 in registers, through contract_backward into three stores.  Lanes past the end take
// part in the shuffles and add nothing.  It reads nothing the forward wrote.  The private arrays of the generic backward (and their
// scratch) are inherited.
// 64-bit entry offsets throughout; no workspace; nothing but the caller's buffers is written.
#include "lp_column_mlp.h"
#include "lp_generic_decode.h"
#include "lp_hash_levels.h"

namespace lp {

// (hp_features, the level loop of both kernels: lp_hash_levels.h)

struct HpFwdArgs {
  LpHashGridArgs g;  // layout, table, points, grid_idx, flags
  LpMlp trunk, opacity, color;
  const float* mlp_params;
  const float* encoding;
  const float* scaffold;
  LpGrid scaffold_shape;
  float* opacity_out;
  float* color_out;
  int64_t n_points;
  int32_t encoding_dim, color_chn;
  float gain;
  int32_t maxw;  // rows of one activation tile
};

template <bool OPACITY_ONLY>
__global__ void __launch_bounds__(SC_WAVE) hash_points_fwd(const HpFwdArgs s) {
  extern __shared__ __attribute__((aligned(16))) float lds[];  // activation tiles [maxw][64]: two, or three with the colour head
  const LpHashGridArgs& g = s.g;
  const int lane = threadIdx.x;
  const int64_t p = (int64_t)blockIdx.x * SC_WAVE + lane;
  const bool valid = p < s.n_points;
  const int64_t q = valid ? p : 0;  // (a lane past the end works on point 0 and stores nothing)
  const int64_t r = q / g.n_pts;
  const HgPoint pt = hg_point(g, q);
  float occ = 1.0f;
  if (s.scaffold) occ = scaffold_lookup(s.scaffold, s.scaffold_shape, pt.ray.b, pt.x, pt.y, pt.z);

  const int C = g.n_levels * g.features_per_level;
  float* cur = lds + lane;
  float* nxt = lds + s.maxw * SC_WAVE + lane;
  hp_features<SC_WAVE>(g, pt, cur);
  if (s.trunk.n_layers == 0) {  // the heads read ReLU(features)
    for (int c = 0; c < C; ++c) cur[c * SC_WAVE] = fmaxf(cur[c * SC_WAVE], 0.0f);
  }
  int hw = C;  // width of the heads' input
  for (int l = 0; l < s.trunk.n_layers; ++l) {
    sc_dense(mlp_w(s.mlp_params, s.trunk, l), mlp_b(s.mlp_params, s.trunk, l), s.trunk.dims[l], s.trunk.dims[l + 1], s.trunk.dims[l + 1],
             cur, nxt, true);
    hw = s.trunk.dims[l + 1];
    float* t = cur;
    cur = nxt;
    nxt = t;
  }
  float* cin = lds + 2 * s.maxw * SC_WAVE + lane;  // the colour head's input (third tile; not there when OPACITY_ONLY)
  if (!OPACITY_ONLY) {
    const float* e = s.encoding + r * s.encoding_dim;
    for (int c = 0; c < hw; ++c) cin[c * SC_WAVE] = cur[c * SC_WAVE] + e[c];
  }
  for (int l = 0; l < s.opacity.n_layers; ++l) {
    const bool last = l == s.opacity.n_layers - 1;
    sc_dense(mlp_w(s.mlp_params, s.opacity, l), mlp_b(s.mlp_params, s.opacity, l), s.opacity.dims[l], s.opacity.dims[l + 1],
             last ? 1 : s.opacity.dims[l + 1], cur, nxt, !last);
    float* t = cur;
    cur = nxt;
    nxt = t;
  }
  const float opacity = s.gain * softplus_f(cur[0]) * occ;
  if (valid) s.opacity_out[p] = opacity;
  if (!OPACITY_ONLY) {
    cur = cin;  // (both other tiles are free now)
    for (int l = 0; l < s.color.n_layers; ++l) {
      const bool last = l == s.color.n_layers - 1;
      sc_dense(mlp_w(s.mlp_params, s.color, l), mlp_b(s.mlp_params, s.color, l), s.color.dims[l], s.color.dims[l + 1],
               last ? s.color_chn : s.color.dims[l + 1], cur, nxt, !last);
      float* t = cur;
      cur = nxt;
      nxt = t;
    }
    if (valid) {
      float* out = s.color_out + p * s.color_chn;
      for (int c = 0; c < s.color_chn; ++c) out[c] = sigmoid_f(cur[c * SC_WAVE]) * occ;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------------------------------------

struct HpBwdArgs {
  GenArgs ga;              // the decoder and its result gradients in the generic Renderer's argument block (grid-list: channels only)
  LpHashGridArgs g;        // layout, table, points, grid_idx, flags; grad_table and grad_points: results or NULL
  const float* g_opacity;  // [n_points] or NULL
  const float* g_color;    // [n_points, color_chn]; non-NULL exactly when `color`
  int64_t n_points;
  int32_t tiles_per_block;  // consecutive 64-point tiles of one workgroup
  int32_t color;            // the colour head takes part
};
static_assert(sizeof(HpBwdArgs) <= 4096, "a kernel's argument block has at most 4 KB");

// one level of the backward: d = the lane's d feat[l F ..] (used when `on`).  Every lane of the wave calls this.
template <int F>
LP_DEV void hp_level_b(const LpHashGridArgs& g, const HgPoint& pt, const HgLevel& lv, const float* d, bool on, int lane, float& gx,
                       float& gy, float& gz) {
  HgRow<F> dl;
#pragma unroll
  for (int c = 0; c < F; ++c) dl.v[c] = on ? d[c] : 0.0f;
  if (g.grad_table) {
    const HgCell cell = hg_cell(pt, lv);
    const HgRun run = hg_run(cell, pt.ray.b, on, lane);
    hg_table_grad<F>(g.grad_table + hg_base(g, pt.ray.b, lv, F), cell, lv, dl, on, run);
  }
  if (g.grad_points && on) hg_point_grad<F>(g, pt, lv, dl.v, gx, gy, gz);
}

template <int ACT_CAP, bool LDS_ACC>
__global__ void __launch_bounds__(64) hash_points_bwd(const HpBwdArgs s) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const GenArgs& ga = s.ga;
  const LpRendererArgs& a = ga.a;
  const GenPlan& p = ga.p;
  const LpHashGridArgs& g = s.g;
  const int lane = threadIdx.x;

  float* Xs = lds;
  float* Ys = lds + 64 * ga.stage_ld;
  float* gparams_lds = lds + 128 * ga.stage_ld;
  float* gparams = nullptr;
  if (a.grad_mlp_params) {
    if (LDS_ACC) {
      for (int64_t i = lane; i < a.n_mlp_params; i += 64) gparams_lds[i] = 0.0f;
      gparams = gparams_lds;
    } else {
      gparams = a.grad_mlp_params;
    }
  }
  __syncthreads();

  float act[ACT_CAP];
  float enc[LP_MAX_WIDTH];
  float dy[LP_MAX_WIDTH], dx[LP_MAX_WIDTH], dhead[LP_MAX_WIDTH];
  const int E = a.rays.encoding_dim;
  const int Cc = a.color_chn;
  const bool color = s.color != 0;  // wave-uniform
  const int C = a.grid.channels;    // L F
  const int F = g.features_per_level;
  const int hw = p.head_w;
  const int craw = color ? p.col[a.color.n_layers - 1] : 0;
  const int64_t n_tiles = (s.n_points + 63) / 64;

  for (int t = 0; t < s.tiles_per_block; ++t) {
    const int64_t tile = (int64_t)blockIdx.x * s.tiles_per_block + t;
    if (tile >= n_tiles) break;  // wave-uniform
    const int64_t first = tile * 64;
    const int64_t left = s.n_points - first;
    const int rows = left < 64 ? (int)left : 64;
    const bool live = lane < rows;
    const int64_t q = live ? first + lane : 0;  // (a lane past the end recomputes point 0 and contributes nothing)
    const int64_t r = q / g.n_pts;
    const HgPoint pt = hg_point(g, q);
    float occ = 1.0f;
    if (a.scaffold) occ = scaffold_lookup(a.scaffold, a.scaffold_shape, pt.ray.b, pt.x, pt.y, pt.z);
    if (color)
      for (int c = 0; c < E; ++c) enc[c] = a.rays.encoding[r * E + c];
    hp_features<1>(g, pt, act + p.x0);
    const float raw = color ? decode_gathered(ga, enc, act, Xs, lane) : decode_opacity_gathered(ga, act, Xs, lane);
    const float g_op = (live && s.g_opacity) ? s.g_opacity[q] : 0.0f;
    const float d_raw_op = g_op * a.gain * occ * d_softplus_f(raw);

    // ---- colour head ----
    if (color) {
      for (int c = 0; c < Cc; ++c) {
        const float sg = sigmoid_f(act[craw + c]);
        dy[c] = live ? s.g_color[q * Cc + c] * occ * sg * (1.0f - sg) : 0.0f;
      }
      mlp_backward<LDS_ACC>(a.mlp_params, ga.stage_ld, a.color, Cc, p.col_in, p.col, act, dy, dx, gparams, Xs, Ys, lane, live);
      for (int c = 0; c < hw; ++c) dhead[c] = dx[c];
      if (a.grad_encoding) encoding_grad_wave(a.grad_encoding, E, dx, live, first, g.n_pts, rows, Xs, ga.stage_ld, lane);
    } else {
      for (int c = 0; c < hw; ++c) dhead[c] = 0.0f;
    }
    // ---- opacity head ----
    dy[0] = d_raw_op;
    mlp_backward<LDS_ACC>(a.mlp_params, ga.stage_ld, a.opacity, 1, p.op_in, p.op, act, dy, dx, gparams, Xs, Ys, lane, live);
    // ---- trunk: its output gradient = colour-input grad + opacity-input grad, through the ReLU ----
    for (int c = 0; c < hw; ++c) {
      const float gsum = dhead[c] + dx[c];
      dy[c] = (act[p.op_in + c] > 0.0f) ? gsum : 0.0f;
    }
    if (a.trunk.n_layers > 0) {
      const LpMlp& m = a.trunk;
      mlp_backward<LDS_ACC>(a.mlp_params, ga.stage_ld, m, m.dims[m.n_layers], p.x0, p.trunk, act, dy, dx, gparams, Xs, Ys, lane, live);
    } else {
      for (int c = 0; c < C; ++c) dx[c] = dy[c];
    }
    // ---- the levels: dx = d feat ----
    if (g.grad_table || g.grad_points) {
      const bool on = live && pt.inside;
      float gx = 0.0f, gy = 0.0f, gz = 0.0f;
      for (int l = 0; l < g.n_levels; ++l) {
        const HgLevel lv = hg_level(g, l);
        const float* d = dx + l * F;
        switch (F) {
          case 1: hp_level_b<1>(g, pt, lv, d, on, lane, gx, gy, gz); break;
          case 2: hp_level_b<2>(g, pt, lv, d, on, lane, gx, gy, gz); break;
          case 4: hp_level_b<4>(g, pt, lv, d, on, lane, gx, gy, gz); break;
          default: hp_level_b<8>(g, pt, lv, d, on, lane, gx, gy, gz); break;
        }
      }
      if (g.grad_points) {
        if (on && g.contract_coords) contract_backward(pt.ray.ox, pt.ray.oy, pt.ray.oz, gx, gy, gz);
        if (live) {
          float* gp = g.grad_points + 3 * q;
          gp[0] = gx;
          gp[1] = gy;
          gp[2] = gz;
        }
      }
    }
  }
  if (LDS_ACC && a.grad_mlp_params) {
    __syncthreads();
    for (int64_t i = lane; i < a.n_mlp_params; i += 64) {
      const float v = gparams_lds[i];
      if (v != 0.0f) atomic_add_f32(a.grad_mlp_params + i, v);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// host side (`a` checked by lp_api.hip)
// ---------------------------------------------------------------------------------------------------------------------------

constexpr int64_t HP_BWD_BLOCKS = 2048;  // workgroups a large backward is cut into, as points_bwd

// the layout, the table and the points as the level functions (and the layout check of lp_api.hip) read them
LpHashGridArgs hash_points_view(const LpHashPointsArgs& a) {
  LpHashGridArgs g = {};
  g.table = a.table;
  g.grad_table = a.grad_table;
  g.points = a.points;
  g.grid_idx = a.grid_idx;
  g.grad_points = a.grad_points;
  g.entries = a.entries;
  g.n_rays = a.n_rays;
  g.n_pts = a.n_pts;
  for (int l = 0; l < LP_HASH_MAX_LEVELS; ++l) {
    g.offset[l] = a.offset[l];
    g.resolution[l] = a.resolution[l];
    g.size[l] = a.size[l];
    g.hashed[l] = a.hashed[l];
  }
  g.batch = a.batch;
  g.features_per_level = a.features_per_level;
  g.n_levels = a.n_levels;
  g.mask_out_of_bounds = a.mask_out_of_bounds;
  g.contract_coords = a.contract_coords;
  return g;
}

int hash_points_forward_launch(const LpHashPointsArgs& a, hipStream_t stream) {
  HpFwdArgs s;
  s.g = hash_points_view(a);
  s.n_points = a.n_rays * a.n_pts;
  if (s.n_points == 0) return LP_OK;
  const bool opacity_only = a.color_out == nullptr;
  s.trunk = a.trunk, s.opacity = a.opacity, s.color = a.color;
  s.mlp_params = a.mlp_params;
  s.encoding = a.encoding;
  s.scaffold = a.scaffold;
  s.scaffold_shape = a.scaffold_shape;
  s.opacity_out = a.opacity_out;
  s.color_out = a.color_out;
  s.encoding_dim = a.encoding_dim;
  s.color_chn = a.color_chn;
  s.gain = a.gain;
  int maxw = a.n_levels * a.features_per_level;
  const LpMlp* ms[3] = {&a.trunk, &a.opacity, &a.color};
  for (int k = 0; k < (opacity_only ? 2 : 3); ++k)
    for (int l = 0; l <= ms[k]->n_layers && ms[k]->n_layers > 0; ++l) maxw = ms[k]->dims[l] > maxw ? ms[k]->dims[l] : maxw;
  s.maxw = maxw;
  const size_t lds = (size_t)(opacity_only ? 2 : 3) * maxw * SC_WAVE * sizeof(float);  // <= 96 KB (LP_MAX_WIDTH 128)
  unsigned blocks;
  if (int rc = launch_blocks("lp_hash_points_forward", s.n_points, SC_WAVE, blocks)) return rc;
  const void* fn = opacity_only ? (const void*)hash_points_fwd<true> : (const void*)hash_points_fwd<false>;
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return set_error((int)e, "hipFuncSetAttribute: %s", hipGetErrorString(e));
  const dim3 gr(blocks), bl(SC_WAVE);
  if (opacity_only)
    hipLaunchKernelGGL((hash_points_fwd<true>), gr, bl, lds, stream, s);
  else
    hipLaunchKernelGGL((hash_points_fwd<false>), gr, bl, lds, stream, s);
  return check_launch("hash_points_fwd");
}

// the generic Renderer's argument block of the decoder: no grid-list, `channels` features
static void decoder_view(const LpHashPointsArgs& a, bool color, LpRendererArgs& ra) {
  ra = LpRendererArgs{};
  ra.rays.n_rays = a.n_rays;
  ra.rays.grid_idx = a.grid_idx;
  ra.rays.encoding = a.encoding;
  ra.rays.encoding_dim = color ? a.encoding_dim : 0;
  ra.grid.channels = a.n_levels * a.features_per_level;
  ra.scaffold = a.scaffold;
  ra.scaffold_shape = a.scaffold_shape;
  ra.march.num_samples = 1;
  ra.march.mask_out_of_bounds = a.mask_out_of_bounds;
  ra.march.contract_coords = a.contract_coords;
  ra.mlp_params = a.mlp_params;
  ra.n_mlp_params = a.n_mlp_params;
  ra.trunk = a.trunk;
  ra.opacity = a.opacity;
  ra.color = a.color;
  if (!color) ra.color.n_layers = 0;
  ra.color_chn = a.color_chn;
  ra.gain = a.gain;
  ra.grad_mlp_params = a.grad_mlp_params;
  ra.grad_encoding = color ? a.grad_encoding : nullptr;
}

int hash_points_backward_total_width(const LpHashPointsArgs& a) {
  LpRendererArgs ra;
  decoder_view(a, a.grad_color != nullptr, ra);
  GenPlan p;
  return make_plan(ra, p);
}

int hash_points_backward_launch(const LpHashPointsArgs& a, hipStream_t stream) {
  HpBwdArgs s;
  const bool color = a.grad_color != nullptr;
  decoder_view(a, color, s.ga.a);
  const LpRendererArgs& ra = s.ga.a;
  s.g = hash_points_view(a);
  s.n_points = a.n_rays * a.n_pts;
  if (s.n_points == 0) return LP_OK;
  if (!a.grad_opacity && !a.grad_color) return LP_OK;  // both upstream gradients are zero: so is every result (buffers are zeroed)
  const int total = make_plan(ra, s.ga.p);  // (<= 1024: lp_api.hip)
  s.ga.stage_ld = generic_stage_ld(ra);
  s.ga.relu_dump = nullptr;
  s.ga.dump_words = s.ga.dump_wps = 0;
  s.g_opacity = a.grad_opacity;
  s.g_color = a.grad_color;
  s.color = color ? 1 : 0;
  const size_t stage_bytes = (size_t)128 * s.ga.stage_ld * sizeof(float);
  const size_t param_bytes = (size_t)a.n_mlp_params * sizeof(float);
  const bool lds_acc = a.grad_mlp_params && (stage_bytes + param_bytes <= 96 * 1024);
  s.ga.lds_param_accum = lds_acc ? 1 : 0;
  const size_t lds = stage_bytes + (lds_acc ? param_bytes : 0);
  // n_tiles tiles of 64 points, dealt to at most HP_BWD_BLOCKS workgroups of tpb consecutive tiles
  int64_t n_tiles, tpb;
  workgroup_count(s.n_points, 64, n_tiles);
  workgroup_count(n_tiles, HP_BWD_BLOCKS, tpb);  // (n_points < 2^31: it fits)
  s.tiles_per_block = (int32_t)tpb;
  unsigned blocks;
  if (int rc = launch_blocks("lp_hash_points_backward", n_tiles, tpb, blocks)) return rc;
#define LP_LAUNCH_HP_BWD(CAP, ACC)                                                                                                    \
  do {                                                                                                                                \
    hipError_t e = hipFuncSetAttribute((const void*)hash_points_bwd<CAP, ACC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    if (e != hipSuccess) return set_error((int)e, "hipFuncSetAttribute: %s", hipGetErrorString(e));                                   \
    hipLaunchKernelGGL((hash_points_bwd<CAP, ACC>), dim3(blocks), dim3(64), lds, stream, s);                                          \
  } while (0)
  if (total <= 256) {
    if (lds_acc) LP_LAUNCH_HP_BWD(256, true); else LP_LAUNCH_HP_BWD(256, false);
  } else {
    if (lds_acc) LP_LAUNCH_HP_BWD(1024, true); else LP_LAUNCH_HP_BWD(1024, false);
  }
#undef LP_LAUNCH_HP_BWD
  return check_launch("hash_points_bwd");
}

}  // namespace lp

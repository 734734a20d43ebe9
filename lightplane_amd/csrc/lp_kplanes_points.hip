// lp_kplanes_points.hip -- the decoder on a space-time plane field (K-Planes / HexPlane; without time planes the Hadamard tri-plane) at
// 3-D points, encoding and decoder in one launch (C ABI lp_kplanes_points_forward / lp_kplanes_points_backward,
// include/lightplane_hip_kplanes_points.h, which holds the definition).  The features [n_rays, n_pts, S C] of the chain
// kplanes_encode -> decoder never reach memory, and neither does their gradient.
//
// A point reads 4 P S rows of 4 C bytes (96 rows of 128 bytes at C = 32, dynamic, four scales): the gather and the scatter want
// lanes = channels, so that a row is one coalesced access; the decoder wants lane = point with the activations in an LDS column tile.
// Both kernels carry both mappings in one workgroup (one wave, 64 consecutive points) and transpose between them in LDS.
//
// Forward, kplanes_points_fwd<P, OPACITY_ONLY>, three phases per workgroup:
//   1  lane = point: the point's geometry, the scaffold's value, and per scale the tile geo[64][4 P + 1] (kp_tile_store: per plane the
//      64-bit base row and the two fractions; a masked point or a lane past the end leaves a negative row).  The tile lies in the
//      decoder's SECOND activation tile, which is not live before the first layer runs; the tiles have max(maxw, 4 P + 1) rows, so a
//      decoder narrower than the geometry still holds it.
//   2  lanes = channels (kpp_gather): C / 4 consecutive lanes serve one point with a float4 of channels each, 256 / C points per
//      pass, C / 4 passes per scale.  A lane issues its 4 P loads of 16 bytes before the first use -- the C / 4 lanes of a point read
//      whole rows of 4 C bytes --, folds them into the P bilinear values, multiplies those (the arithmetic and the order of
//      kplanes_fwd: the same bits) and writes its four products to rows s C + c .. of the first column tile [rows][64].
//      LDS WRITE PATTERN: element (row i, point p) sits at word 64 i + p, so the bank is p mod 32 whatever the channel: the lanes of
//      one point always collide.  With float4 slices a write instruction has C / 4 lanes per point: a C / 4-way conflict (none at
//      C = 4, 2-way at 8, 8-way at 32, 16-way at 64), C passes of 32-lane halves per scale and tile where single channels per lane
//      (C lanes per point, C-way conflicts) would take 4 C.  The reads of geo are broadcasts within a point and conflict-free between
//      points (odd stride).
//   3  lane = point: trunk and heads are the body of hash_points_fwd (sc_dense, two tiles ping-ponging, a third for the colour
//      head's input).  No private array, no scratch, no atomics: bit-reproducible.
//
// Backward, kplanes_points_bwd<P, ACT_CAP, LDS_ACC>: one launch; a workgroup (one wave) takes a run of consecutive 64-point tiles and
// reads nothing the forward wrote.  LDS: Xs[64][ld] | Ys[64][ld] (the staging tiles of the generic backward, ld = max(widest layer
// + 1, 4 P + 1)) | pg[64][3] | the weight-gradient accumulators when they fit.  Per tile:
//   recompute   per scale, geo into Ys (phase 1), kpp_gather into Xs as [point][ld] (a point's lanes write consecutive words); then
//               lane = point copies its row into act + p.x0.
//   decoder     decode_gathered / decode_opacity_gathered, mlp_backward through the colour head, the opacity head and the trunk,
//               encoding_grad_wave: exactly hash_points_bwd.  That leaves d feat[S C] per lane.
//   transpose   d feat is staged into Xs as [64][ld] (zeros for a masked point or a lane past the end).
//   walk        per scale, geo into Ys again, then kpp_walk, lanes = channels: groups of C lanes walk C consecutive points (64 / C
//               groups side by side), reload the four vertices per plane, form the product of the other planes by the prefix /
//               suffix pass (no division), keep four vertex sums per plane in registers and add them to grad_planes -- whole rows,
//               fp32 atomics -- only when that plane's base row changes (run merging per plane, as kplanes_bwd_planes).  In the same
//               walk every lane forms its channel's share of sum_j (d v_j / d axis) o_j from the taps it holds; the group reduces
//               it with xor shuffles and its first lane adds it, times (n_s - 1) / 2 (0 on a clamped axis), to pg[point][axis].
//               After the scales lane = point applies contract_backward and stores three floats: a fixed order, the same bits
//               whichever other gradients are asked for.
// grad_planes == NULL skips the atomics, grad_points == NULL the axis sums, both the walk.  Lanes past the end and masked points take
// part in barriers and shuffles and add nothing.  The private arrays of the generic backward (and their scratch) are inherited.
// 64-bit row offsets throughout; no workspace; nothing but the caller's buffers is written.
#include "lp_column_mlp.h"
#include "lp_generic_decode.h"
#include "lp_kplanes_tile.h"

namespace lp {

struct KppFwdArgs {
  LpKPlanesArgs g;  // layout, planes, points, times, grid_idx, flags
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
  int32_t tile_rows;  // rows of one activation tile: max(widest layer, 4 P + 1)
  int32_t lanes_log;  // log2(C / 4): lanes per point of the gather
};

template <int P, bool OPACITY_ONLY>
__global__ void __launch_bounds__(SC_WAVE) kplanes_points_fwd(const KppFwdArgs s) {
  extern __shared__ __attribute__((aligned(16))) float lds[];  // activation tiles [tile_rows][64]: two, or three with the colour head
  const LpKPlanesArgs& g = s.g;
  const int lane = threadIdx.x;
  const int64_t p = (int64_t)blockIdx.x * SC_WAVE + lane;
  const bool valid = p < s.n_points;
  const int64_t q = valid ? p : 0;  // (a lane past the end looks at point 0, gathers nothing and stores nothing)
  const int64_t r = q / g.n_pts;
  const KpPoint pt = kp_point<P>(g, q);
  float occ = 1.0f;
  if (s.scaffold) occ = scaffold_lookup(s.scaffold, s.scaffold_shape, pt.ray.b, pt.x, pt.y, pt.z);

  const int C = g.n_scales * g.channels;
  float* tile0 = lds;
  float* tile1 = lds + s.tile_rows * SC_WAVE;
  for (int sc = 0; sc < g.n_scales; ++sc) {
    kp_tile_store<P>(g, kp_cell<P>(g, pt, sc), pt.ray.b, sc, valid && pt.inside, tile1 + lane * KP_LD(P));
    __syncthreads();
    kpp_gather<P>(g, tile1, sc, s.lanes_log, lane, tile0, 1, SC_WAVE);
    __syncthreads();
  }
  float* cur = tile0 + lane;
  float* nxt = tile1 + lane;
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
  float* cin = lds + 2 * s.tile_rows * SC_WAVE + lane;  // the colour head's input (third tile; not there when OPACITY_ONLY)
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

struct KppBwdArgs {
  GenArgs ga;              // the decoder and its result gradients in the generic Renderer's argument block (grid-list: channels only)
  LpKPlanesArgs g;         // layout, planes, points, times, grid_idx, flags; grad_planes and grad_points: results or NULL
  const float* g_opacity;  // [n_points] or NULL
  const float* g_color;    // [n_points, color_chn]; non-NULL exactly when `color`
  int64_t n_points;
  int32_t tiles_per_block;  // consecutive 64-point tiles of one workgroup
  int32_t color;            // the colour head takes part
  int32_t lanes_log;        // log2(C / 4): lanes per point of the gather
  int32_t cw_log;           // log2(C): lanes of a group of the walk
};
static_assert(sizeof(KppBwdArgs) <= 4096, "a kernel's argument block has at most 4 KB");

template <int P, int ACT_CAP, bool LDS_ACC>
__global__ void __launch_bounds__(64) kplanes_points_bwd(const KppBwdArgs s) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const GenArgs& ga = s.ga;
  const LpRendererArgs& a = ga.a;
  const GenPlan& p = ga.p;
  const LpKPlanesArgs& g = s.g;
  const int lane = threadIdx.x;
  const int ld = ga.stage_ld;  // >= S C + 1 and >= KP_LD(P)

  float* Xs = lds;
  float* Ys = lds + 64 * ld;
  float* pg = lds + 128 * ld;  // [64][3]
  float* gparams_lds = pg + 192;
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
  const int C = a.grid.channels;    // S C
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
    const int64_t q = live ? first + lane : 0;  // (a lane past the end looks at point 0 and contributes nothing)
    const int64_t r = q / g.n_pts;
    const KpPoint pt = kp_point<P>(g, q);
    const bool on = live && pt.inside;
    float occ = 1.0f;
    if (a.scaffold) occ = scaffold_lookup(a.scaffold, a.scaffold_shape, pt.ray.b, pt.x, pt.y, pt.z);
    if (color)
      for (int c = 0; c < E; ++c) enc[c] = a.rays.encoding[r * E + c];
    // ---- recompute: geometry by lane = point, gather by lanes = channels into Xs[point][ld], back to lane = point ----
    for (int sc = 0; sc < g.n_scales; ++sc) {
      kp_tile_store<P>(g, kp_cell<P>(g, pt, sc), pt.ray.b, sc, on, Ys + lane * KP_LD(P));
      __syncthreads();
      kpp_gather<P>(g, Ys, sc, s.lanes_log, lane, Xs, ld, 1);
      __syncthreads();
    }
    for (int c = 0; c < C; ++c) act[p.x0 + c] = Xs[lane * ld + c];
    __syncthreads();
    const float raw = color ? decode_gathered(ga, enc, act, Xs, lane) : decode_opacity_gathered(ga, act, Xs, lane);
    const float g_op = (live && s.g_opacity) ? s.g_opacity[q] : 0.0f;
    const float d_raw_op = g_op * a.gain * occ * d_softplus_f(raw);

    // ---- colour head ----
    if (color) {
      for (int c = 0; c < Cc; ++c) {
        const float sg = sigmoid_f(act[craw + c]);
        dy[c] = live ? s.g_color[q * Cc + c] * occ * sg * (1.0f - sg) : 0.0f;
      }
      mlp_backward<LDS_ACC>(a.mlp_params, ld, a.color, Cc, p.col_in, p.col, act, dy, dx, gparams, Xs, Ys, lane, live);
      for (int c = 0; c < hw; ++c) dhead[c] = dx[c];
      if (a.grad_encoding) encoding_grad_wave(a.grad_encoding, E, dx, live, first, g.n_pts, rows, Xs, ld, lane);
    } else {
      for (int c = 0; c < hw; ++c) dhead[c] = 0.0f;
    }
    // ---- opacity head ----
    dy[0] = d_raw_op;
    mlp_backward<LDS_ACC>(a.mlp_params, ld, a.opacity, 1, p.op_in, p.op, act, dy, dx, gparams, Xs, Ys, lane, live);
    // ---- trunk: its output gradient = colour-input grad + opacity-input grad, through the ReLU ----
    for (int c = 0; c < hw; ++c) {
      const float gsum = dhead[c] + dx[c];
      dy[c] = (act[p.op_in + c] > 0.0f) ? gsum : 0.0f;
    }
    if (a.trunk.n_layers > 0) {
      const LpMlp& m = a.trunk;
      mlp_backward<LDS_ACC>(a.mlp_params, ld, m, m.dims[m.n_layers], p.x0, p.trunk, act, dy, dx, gparams, Xs, Ys, lane, live);
    } else {
      for (int c = 0; c < C; ++c) dx[c] = dy[c];
    }
    // ---- the planes: dx = d feat goes to lanes = channels through Xs ----
    if (g.grad_planes || g.grad_points) {
      __syncthreads();
      stage(Xs, ld, lane, dx, C, !on);
      if (g.grad_points) pg[3 * lane] = pg[3 * lane + 1] = pg[3 * lane + 2] = 0.0f;
      for (int sc = 0; sc < g.n_scales; ++sc) {
        kp_tile_store<P>(g, kp_cell<P>(g, pt, sc), pt.ray.b, sc, on, Ys + lane * KP_LD(P));
        __syncthreads();
        kpp_walk<P>(g, Ys, Xs, ld, sc, s.cw_log, lane, pg);
        __syncthreads();
      }
      if (g.grad_points) {
        float gx = pg[3 * lane], gy = pg[3 * lane + 1], gz = pg[3 * lane + 2];
        if (on && g.contract_coords) contract_backward(pt.ray.ox, pt.ray.oy, pt.ray.oz, gx, gy, gz);
        if (live) {
          float* gp = g.grad_points + 3 * q;
          gp[0] = gx;
          gp[1] = gy;
          gp[2] = gz;
        }
      }
      __syncthreads();
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

constexpr int64_t KPP_BWD_BLOCKS = 2048;  // workgroups a large backward is cut into, as hash_points_bwd

static int kpp_log2(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

// the layout, the planes, the points and the timestamps as the plane helpers (and the layout check of lp_api.hip) read them
LpKPlanesArgs kplanes_points_view(const LpKPlanesPointsArgs& a) {
  LpKPlanesArgs g = {};
  g.planes = a.planes;
  g.grad_planes = a.grad_planes;
  g.points = a.points;
  g.times = a.times;
  g.grid_idx = a.grid_idx;
  g.grad_points = a.grad_points;
  g.rows = a.rows;
  g.n_rays = a.n_rays;
  g.n_pts = a.n_pts;
  for (int s = 0; s < LP_KPLANES_MAX_SCALES; ++s) {
    for (int j = 0; j < LP_KPLANES_MAX_PLANES; ++j) g.offset[s][j] = a.offset[s][j];
    g.spatial[s] = a.spatial[s];
    g.temporal[s] = a.temporal[s];
  }
  g.batch = a.batch;
  g.channels = a.channels;
  g.n_scales = a.n_scales;
  g.n_planes = a.n_planes;
  g.time_per_point = a.time_per_point;
  g.mask_out_of_bounds = a.mask_out_of_bounds;
  g.contract_coords = a.contract_coords;
  return g;
}

int kplanes_points_forward_launch(const LpKPlanesPointsArgs& a, hipStream_t stream) {
  KppFwdArgs s;
  s.g = kplanes_points_view(a);
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
  s.lanes_log = kpp_log2(a.channels / 4);
  int maxw = a.n_scales * a.channels;
  const LpMlp* ms[3] = {&a.trunk, &a.opacity, &a.color};
  for (int k = 0; k < (opacity_only ? 2 : 3); ++k)
    for (int l = 0; l <= ms[k]->n_layers && ms[k]->n_layers > 0; ++l) maxw = ms[k]->dims[l] > maxw ? ms[k]->dims[l] : maxw;
  const int geo = KP_LD(a.n_planes);  // the geometry tile [64][4 P + 1] lies in the second activation tile
  s.tile_rows = maxw > geo ? maxw : geo;
  const size_t lds = (size_t)(opacity_only ? 2 : 3) * s.tile_rows * SC_WAVE * sizeof(float);  // <= 96 KB (LP_MAX_WIDTH 128)
  unsigned blocks;
  if (int rc = launch_blocks("lp_kplanes_points_forward", s.n_points, SC_WAVE, blocks)) return rc;
#define LP_LAUNCH_KPP_FWD(P, OO)                                                                                                       \
  do {                                                                                                                                 \
    hipError_t e = hipFuncSetAttribute((const void*)kplanes_points_fwd<P, OO>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    if (e != hipSuccess) return set_error((int)e, "hipFuncSetAttribute: %s", hipGetErrorString(e));                                    \
    hipLaunchKernelGGL((kplanes_points_fwd<P, OO>), dim3(blocks), dim3(SC_WAVE), lds, stream, s);                                      \
  } while (0)
  if (a.n_planes == 3) {
    if (opacity_only) LP_LAUNCH_KPP_FWD(3, true); else LP_LAUNCH_KPP_FWD(3, false);
  } else {
    if (opacity_only) LP_LAUNCH_KPP_FWD(6, true); else LP_LAUNCH_KPP_FWD(6, false);
  }
#undef LP_LAUNCH_KPP_FWD
  return check_launch("kplanes_points_fwd");
}

// the generic Renderer's argument block of the decoder: no grid-list, `channels` features
static void kpp_decoder_view(const LpKPlanesPointsArgs& a, bool color, LpRendererArgs& ra) {
  ra = LpRendererArgs{};
  ra.rays.n_rays = a.n_rays;
  ra.rays.grid_idx = a.grid_idx;
  ra.rays.encoding = a.encoding;
  ra.rays.encoding_dim = color ? a.encoding_dim : 0;
  ra.grid.channels = a.n_scales * a.channels;
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

int kplanes_points_backward_total_width(const LpKPlanesPointsArgs& a) {
  LpRendererArgs ra;
  kpp_decoder_view(a, a.grad_color != nullptr, ra);
  GenPlan p;
  return make_plan(ra, p);
}

int kplanes_points_backward_launch(const LpKPlanesPointsArgs& a, hipStream_t stream) {
  KppBwdArgs s;
  const bool color = a.grad_color != nullptr;
  kpp_decoder_view(a, color, s.ga.a);
  const LpRendererArgs& ra = s.ga.a;
  s.g = kplanes_points_view(a);
  s.n_points = a.n_rays * a.n_pts;
  if (s.n_points == 0) return LP_OK;
  if (!a.grad_opacity && !a.grad_color) return LP_OK;  // both upstream gradients are zero: so is every result (buffers are zeroed)
  const int total = make_plan(ra, s.ga.p);  // (<= 1024: lp_api.hip)
  const int geo = KP_LD(a.n_planes);        // the geometry tile [64][4 P + 1] lies in the second staging tile
  const int ld = generic_stage_ld(ra);
  s.ga.stage_ld = ld > geo ? ld : geo;
  s.ga.relu_dump = nullptr;
  s.ga.dump_words = s.ga.dump_wps = 0;
  s.g_opacity = a.grad_opacity;
  s.g_color = a.grad_color;
  s.color = color ? 1 : 0;
  s.lanes_log = kpp_log2(a.channels / 4);
  s.cw_log = kpp_log2(a.channels);
  const size_t stage_bytes = ((size_t)128 * s.ga.stage_ld + 192) * sizeof(float);  // Xs, Ys and the point-gradient sums [64][3]
  const size_t param_bytes = (size_t)a.n_mlp_params * sizeof(float);
  const bool lds_acc = a.grad_mlp_params && (stage_bytes + param_bytes <= 96 * 1024);
  s.ga.lds_param_accum = lds_acc ? 1 : 0;
  const size_t lds = stage_bytes + (lds_acc ? param_bytes : 0);
  // n_tiles tiles of 64 points, dealt to at most KPP_BWD_BLOCKS workgroups of tpb consecutive tiles
  int64_t n_tiles, tpb;
  workgroup_count(s.n_points, 64, n_tiles);
  workgroup_count(n_tiles, KPP_BWD_BLOCKS, tpb);  // (n_points < 2^31: it fits)
  s.tiles_per_block = (int32_t)tpb;
  unsigned blocks;
  if (int rc = launch_blocks("lp_kplanes_points_backward", n_tiles, tpb, blocks)) return rc;
#define LP_LAUNCH_KPP_BWD(P, CAP, ACC)                                                                                                       \
  do {                                                                                                                                       \
    hipError_t e = hipFuncSetAttribute((const void*)kplanes_points_bwd<P, CAP, ACC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    if (e != hipSuccess) return set_error((int)e, "hipFuncSetAttribute: %s", hipGetErrorString(e));                                          \
    hipLaunchKernelGGL((kplanes_points_bwd<P, CAP, ACC>), dim3(blocks), dim3(64), lds, stream, s);                                           \
  } while (0)
#define LP_LAUNCH_KPP_BWD_P(P)                                                          \
  if (total <= 256) {                                                                   \
    if (lds_acc) LP_LAUNCH_KPP_BWD(P, 256, true); else LP_LAUNCH_KPP_BWD(P, 256, false);   \
  } else {                                                                              \
    if (lds_acc) LP_LAUNCH_KPP_BWD(P, 1024, true); else LP_LAUNCH_KPP_BWD(P, 1024, false); \
  }
  if (a.n_planes == 3) {
    LP_LAUNCH_KPP_BWD_P(3)
  } else {
    LP_LAUNCH_KPP_BWD_P(6)
  }
#undef LP_LAUNCH_KPP_BWD_P
#undef LP_LAUNCH_KPP_BWD
  return check_launch("kplanes_points_bwd");
}

const char* build_info_kplanes_points() {
  return "{\"forward\": \"one wave per 64 points: lane = point forms the geometry into an LDS tile aliasing the second activation "
         "tile; lanes = channels (C / 4 lanes per point, float4 slices, C / 4-way bank conflict on the column-tile write) load whole "
         "rows with 4 P loads in flight and write the product into the first column tile; lane = point decodes with sc_dense; no "
         "scratch, no atomics\", \"backward\": \"one wave per run of 64-point tiles: the same gather staged [point][odd stride] and "
         "copied to the private activations, the generic decoder backward, d feat staged back through LDS, then groups of C lanes "
         "walk consecutive points: prefix / suffix products, four vertex sums per plane in registers, whole-row fp32 atomics where a "
         "plane's base row changes, and the point gradient in the same walk (xor-shuffle sum per group, LDS sums per point, stored)\"}";
}

}  // namespace lp

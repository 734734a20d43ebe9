// lp_points.hip -- the decoder at arbitrary 3-D points, forward and backward (C ABI lp_points_forward / lp_points_backward).
//
// Forward, points_fwd<OPACITY_ONLY>: the lattice kernel of lp_scaffold.hip with the points read from memory.  One lane = one point,
// one wave = one workgroup = 64 consecutive points of the [n_rays, n_pts] array; the ray of a point is point / n_pts (64-bit), so a
// ray boundary may fall anywhere inside a wave.  The lane contracts its point when asked (sample_point: the Renderer's arithmetic),
// looks the scaffold up, gathers the grid-list (sc_gather: the Renderer's corner rows, weights and summation order) and evaluates
// trunk -> {opacity head, colour head(+ encoding)} with runtime layer loops (sc_dense).
//   activations: LDS column tiles [maxw][64] (lp_column_mlp.h): two for the opacity-only kernel, a third one holds the colour head's
//                input while the opacity head ping-pongs through the other two.  No private array: no scratch.
//   weights:     wave-uniform scalar loads; arithmetic: fp32 FMA chains in ascending order.
// A lane past the end works on point 0 and stores nothing.
//
// Backward, points_bwd: the shape-generic Renderer backward (lp_renderer_generic.hip) without the march and the compositing.  One lane
// = one point with private activation arrays; it recomputes the decoder (decode(), lp_generic_decode.h: wide layers on the fp32 matrix
// cores), forms d raw and d craw from the upstream gradients and runs mlp_backward through the colour head, the opacity head and the
// trunk; grid gradients leave through splat_list_wave, weight gradients through wave_outer into LDS accumulators that a workgroup
// flushes once after ALL its tiles (a workgroup takes a run of consecutive 64-point tiles: a flush is n_mlp_params atomics, one per
// 64 points would cost more than the points themselves), the encoding gradient is summed per ray inside the wave and added
// atomically (a ray's points span waves), and the point gradient -- the derivative of the interpolation weights times <corner row, d
// features>, through the Jacobian of the contraction -- is stored per point.  It reads nothing the forward wrote.
#include "lp_column_mlp.h"
#include "lp_generic_decode.h"
#include "lp_point_grad.h"

namespace lp {

struct PtFwdArgs {
  LpPointsArgs a;  // normalised: every grid carries its base pointer
  int64_t n_points;
  int32_t maxw;    // rows of one activation tile
};

template <bool OPACITY_ONLY>
__global__ void __launch_bounds__(SC_WAVE) points_fwd(const PtFwdArgs s) {
  extern __shared__ __attribute__((aligned(16))) float lds[];  // activation tiles [maxw][64]: two, or three with the colour head
  const LpPointsArgs& a = s.a;
  const int lane = threadIdx.x;
  const int64_t p = (int64_t)blockIdx.x * SC_WAVE + lane;
  const bool valid = p < s.n_points;
  const int64_t q = valid ? p : 0;
  const int64_t r = q / a.n_pts;
  const int b = clamp_batch(a.grid_idx[r], a.grid.grids[0].B);
  const Ray ray = point_ray(a.points, q, b);
  float x, y, z;
  sample_point(ray, 0.0f, a.contract_coords != 0, x, y, z);
  float occ = 1.0f;
  if (a.scaffold) occ = scaffold_lookup(a.scaffold, a.scaffold_shape, b, x, y, z);

  const bool mask = a.mask_out_of_bounds != 0;
  const int C = a.grid.channels;
  float* cur = lds + lane;
  float* nxt = lds + s.maxw * SC_WAVE + lane;
  sc_gather(a.grid, b, x, y, z, mask, cur);
  if (a.trunk.n_layers == 0) {  // the heads read ReLU(features)
    for (int c = 0; c < C; ++c) cur[c * SC_WAVE] = fmaxf(cur[c * SC_WAVE], 0.0f);
  }
  int hw = C;  // width of the heads' input
  for (int l = 0; l < a.trunk.n_layers; ++l) {
    sc_dense(mlp_w(a.mlp_params, a.trunk, l), mlp_b(a.mlp_params, a.trunk, l), a.trunk.dims[l], a.trunk.dims[l + 1],
             a.trunk.dims[l + 1], cur, nxt, true);
    hw = a.trunk.dims[l + 1];
    float* t = cur;
    cur = nxt;
    nxt = t;
  }
  float* cin = lds + 2 * s.maxw * SC_WAVE + lane;  // the colour head's input (third tile; not touched when OPACITY_ONLY)
  if (!OPACITY_ONLY) {
    const float* e = a.encoding + r * a.encoding_dim;
    if (a.color_grid.n_grids > 0) {
      sc_gather(a.color_grid, b, x, y, z, mask, cin);
      for (int c = 0; c < C; ++c) cin[c * SC_WAVE] = fmaxf(cin[c * SC_WAVE], 0.0f) + e[c];
    } else {
      for (int c = 0; c < hw; ++c) cin[c * SC_WAVE] = cur[c * SC_WAVE] + e[c];
    }
  }
  for (int l = 0; l < a.opacity.n_layers; ++l) {
    const bool last = l == a.opacity.n_layers - 1;
    sc_dense(mlp_w(a.mlp_params, a.opacity, l), mlp_b(a.mlp_params, a.opacity, l), a.opacity.dims[l], a.opacity.dims[l + 1],
             last ? 1 : a.opacity.dims[l + 1], cur, nxt, !last);
    float* t = cur;
    cur = nxt;
    nxt = t;
  }
  const float opacity = a.gain * softplus_f(cur[0]) * occ;
  if (valid) a.opacity_out[p] = opacity;
  if (!OPACITY_ONLY) {
    cur = cin;  // (both other tiles are free now)
    for (int l = 0; l < a.color.n_layers; ++l) {
      const bool last = l == a.color.n_layers - 1;
      sc_dense(mlp_w(a.mlp_params, a.color, l), mlp_b(a.mlp_params, a.color, l), a.color.dims[l], a.color.dims[l + 1],
               last ? a.color_chn : a.color.dims[l + 1], cur, nxt, !last);
      float* t = cur;
      cur = nxt;
      nxt = t;
    }
    if (valid) {
      float* out = a.color_out + p * a.color_chn;
      for (int c = 0; c < a.color_chn; ++c) out[c] = sigmoid_f(cur[c * SC_WAVE]) * occ;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------------------------------------

struct PtBwdArgs {
  GenArgs ga;              // the decoder, the grids and the result gradients in the generic Renderer's argument block
  const float* points;     // [n_points, 3]
  const float* g_opacity;  // [n_points] or NULL
  const float* g_color;    // [n_points, color_chn]; non-NULL exactly when `color`
  float* grad_points;      // [n_points, 3] or NULL
  int64_t n_pts, n_points;
  int32_t tiles_per_block;  // consecutive 64-point tiles of one workgroup
  int32_t color;            // the colour head takes part
};

// grad_encoding[ray] += sum of dx over the ray's points inside this tile.  The lanes' dx go through the tile Xs[64][ld]; then lanes =
// channels walk the tile's rows, which are consecutive points, and add a run's sum when the ray changes: (rays in the tile) x E atomics
// instead of 64 x E on a handful of addresses.  first: the tile's first point; rows: its points inside the array.  Wave-uniform.
LP_DEV void encoding_grad_wave(float* genc, int E, const float* dx, bool live, int64_t first, int64_t n_pts, int rows, float* Xs, int ld,
                               int lane) {
  stage(Xs, ld, lane, dx, E, !live);
  __syncthreads();
  const int64_t r0 = first / n_pts;
  const int64_t rem0 = first - r0 * n_pts;
  for (int c = lane; c < E; c += 64) {
    float sum = 0.0f;
    int64_t r = r0, rem = rem0;
    bool pending = false;
    for (int row = 0; row < rows; ++row) {
      sum += Xs[row * ld + c];
      pending = true;
      if (++rem == n_pts) {
        atomic_add_f32(genc + r * E + c, sum);
        sum = 0.0f;
        rem = 0;
        ++r;
        pending = false;
      }
    }
    if (pending) atomic_add_f32(genc + r * E + c, sum);
  }
  __syncthreads();
}

template <int ACT_CAP, bool LDS_ACC>
__global__ void __launch_bounds__(64) points_bwd(const PtBwdArgs s) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const GenArgs& ga = s.ga;
  const LpRendererArgs& a = ga.a;
  const GenPlan& p = ga.p;
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
  const bool contract = a.march.contract_coords != 0;
  const bool mask = a.march.mask_out_of_bounds != 0;
  const bool two_grids = a.color_grid.n_grids > 0;
  const bool color = s.color != 0;  // wave-uniform
  const int C = a.grid.channels;
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
    const int64_t r = q / s.n_pts;
    const Ray ray = point_ray(s.points, q, clamp_batch(a.rays.grid_idx[r], a.grid.grids[0].B));
    float x, y, z;
    sample_point(ray, 0.0f, contract, x, y, z);
    float occ = 1.0f;
    if (a.scaffold) occ = scaffold_lookup(a.scaffold, a.scaffold_shape, ray.b, x, y, z);
    if (color)
      for (int c = 0; c < E; ++c) enc[c] = a.rays.encoding[r * E + c];
    const float raw = color ? decode(ga, ray, x, y, z, enc, act, Xs, lane) : decode_opacity(ga, ray, x, y, z, act, Xs, lane);
    const float g_op = (live && s.g_opacity) ? s.g_opacity[q] : 0.0f;
    const float d_raw_op = g_op * a.gain * occ * d_softplus_f(raw);

    auto scatter = [&](const LpGridList& gl, float* const* grad, const float* d) {
      if (splat_wave_ok(ga.stage_ld))
        splat_list_wave(gl, grad, ray.b, x, y, z, mask, d, live, Xs, Ys, ga.stage_ld, lane);
      else if (live)
        splat_list(gl, grad, ray.b, x, y, z, mask, d);
    };

    // ---- colour head ----
    if (color) {
      for (int c = 0; c < Cc; ++c) {
        const float sg = sigmoid_f(act[craw + c]);
        dy[c] = live ? s.g_color[q * Cc + c] * occ * sg * (1.0f - sg) : 0.0f;
      }
      mlp_backward<LDS_ACC>(a.mlp_params, ga.stage_ld, a.color, Cc, p.col_in, p.col, act, dy, dx, gparams, Xs, Ys, lane, live);
      for (int c = 0; c < hw; ++c) dhead[c] = dx[c];
      if (a.grad_encoding) encoding_grad_wave(a.grad_encoding, E, dx, live, first, s.n_pts, rows, Xs, ga.stage_ld, lane);
    } else {
      for (int c = 0; c < hw; ++c) dhead[c] = 0.0f;
    }
    // ---- opacity head ----
    dy[0] = d_raw_op;
    mlp_backward<LDS_ACC>(a.mlp_params, ga.stage_ld, a.opacity, 1, p.op_in, p.op, act, dy, dx, gparams, Xs, Ys, lane, live);

    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
    if (two_grids) {
      // opacity input = relu(x0), colour input = relu(cx0) + enc
      for (int c = 0; c < C; ++c) dx[c] = (act[p.x0 + c] > 0.0f) ? dx[c] : 0.0f;
      if (a.grad_grid_list[0]) scatter(a.grid, a.grad_grid_list, dx);
      if (s.grad_points) point_grad_list(a.grid, ray.b, x, y, z, mask, dx, gx, gy, gz);
      if (color) {
        for (int c = 0; c < C; ++c) dhead[c] = (act[p.cx0 + c] > 0.0f) ? dhead[c] : 0.0f;
        if (a.grad_color_grid_list[0]) scatter(a.color_grid, a.grad_color_grid_list, dhead);
        if (s.grad_points) point_grad_list(a.color_grid, ray.b, x, y, z, mask, dhead, gx, gy, gz);
      }
    } else {
      // trunk output gradient = colour-input grad + opacity-input grad, through the ReLU
      for (int c = 0; c < hw; ++c) {
        const float g = dhead[c] + dx[c];
        dy[c] = (act[p.op_in + c] > 0.0f) ? g : 0.0f;
      }
      if (a.trunk.n_layers > 0) {
        // (mlp_backward masks hidden outputs only; the trunk's last layer is ReLU'd too: handled just above)
        const LpMlp& m = a.trunk;
        mlp_backward<LDS_ACC>(a.mlp_params, ga.stage_ld, m, m.dims[m.n_layers], p.x0, p.trunk, act, dy, dx, gparams, Xs, Ys, lane, live);
      } else {
        for (int c = 0; c < C; ++c) dx[c] = dy[c];
      }
      if (a.grad_grid_list[0]) scatter(a.grid, a.grad_grid_list, dx);
      if (s.grad_points) point_grad_list(a.grid, ray.b, x, y, z, mask, dx, gx, gy, gz);
    }
    if (s.grad_points) {
      if (contract) contract_backward(ray.ox, ray.oy, ray.oz, gx, gy, gz);
      if (live) {
        float* gp = s.grad_points + 3 * q;
        gp[0] = gx;
        gp[1] = gy;
        gp[2] = gz;
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
// host side
// ---------------------------------------------------------------------------------------------------------------------------

constexpr int64_t PT_BWD_BLOCKS = 2048;  // workgroups a large backward is cut into (two rounds of the chip's one-wave-per-SIMD slots)

static int widest(const LpPointsArgs& a, bool with_color) {
  int maxw = a.grid.channels;
  const LpMlp* ms[3] = {&a.trunk, &a.opacity, &a.color};
  for (int k = 0; k < (with_color ? 3 : 2); ++k)
    for (int l = 0; l <= ms[k]->n_layers && ms[k]->n_layers > 0; ++l) maxw = ms[k]->dims[l] > maxw ? ms[k]->dims[l] : maxw;
  return maxw;
}

// `a` normalised and checked by lp_api.hip
int points_forward_launch(const LpPointsArgs& a, hipStream_t stream) {
  PtFwdArgs s;
  s.a = a;
  s.n_points = a.n_rays * a.n_pts;
  if (s.n_points == 0) return LP_OK;
  const bool opacity_only = a.color_out == nullptr;
  s.maxw = widest(a, !opacity_only);
  const size_t lds = (size_t)(opacity_only ? 2 : 3) * s.maxw * SC_WAVE * sizeof(float);  // <= 96 KB (LP_MAX_WIDTH 128)
  unsigned blocks;
  if (int rc = launch_blocks("lp_points_forward", s.n_points, SC_WAVE, blocks)) return rc;
  const void* fn = opacity_only ? (const void*)points_fwd<true> : (const void*)points_fwd<false>;
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return set_error((int)e, "hipFuncSetAttribute: %s", hipGetErrorString(e));
  const dim3 gr(blocks), bl(SC_WAVE);
  if (opacity_only)
    hipLaunchKernelGGL((points_fwd<true>), gr, bl, lds, stream, s);
  else
    hipLaunchKernelGGL((points_fwd<false>), gr, bl, lds, stream, s);
  return check_launch("points_fwd");
}

// the generic Renderer's argument block of a point evaluation: decoder, grids, scaffold and result gradients
static void renderer_view(const LpPointsArgs& a, bool color, LpRendererArgs& ra) {
  ra = LpRendererArgs{};
  ra.rays.n_rays = a.n_rays;
  ra.rays.grid_idx = a.grid_idx;
  ra.rays.encoding = a.encoding;
  ra.rays.encoding_dim = color ? a.encoding_dim : 0;
  ra.grid = a.grid;
  ra.color_grid = a.color_grid;
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
  ra.grad_encoding = a.grad_encoding;
  for (int g = 0; g < LP_MAX_GRIDS; ++g) {
    ra.grad_grid_list[g] = a.grad_grid_list[g];
    ra.grad_color_grid_list[g] = a.grad_color_grid_list[g];
  }
}

int points_backward_total_width(const LpPointsArgs& a) {
  LpRendererArgs ra;
  renderer_view(a, a.grad_color != nullptr, ra);
  GenPlan p;
  return make_plan(ra, p);
}

int points_backward_launch(const LpPointsArgs& a, hipStream_t stream) {
  PtBwdArgs s;
  const bool color = a.grad_color != nullptr;
  renderer_view(a, color, s.ga.a);
  const LpRendererArgs& ra = s.ga.a;
  s.n_pts = a.n_pts;
  s.n_points = a.n_rays * a.n_pts;
  if (s.n_points == 0) return LP_OK;
  if (!a.grad_opacity && !a.grad_color) return LP_OK;  // both upstream gradients are zero: so is every result (buffers are zeroed)
  const int total = make_plan(ra, s.ga.p);
  if (total > 1024) return set_error(LP_EUNSUPPORTED, "lp_points_backward: sum of layer widths %d exceeds 1024", total);
  s.ga.stage_ld = generic_stage_ld(ra);
  s.ga.relu_dump = nullptr;
  s.ga.dump_words = s.ga.dump_wps = 0;
  s.points = a.points;
  s.g_opacity = a.grad_opacity;
  s.g_color = a.grad_color;
  s.grad_points = a.grad_points;
  s.color = color ? 1 : 0;
  const size_t stage_bytes = (size_t)128 * s.ga.stage_ld * sizeof(float);
  const size_t param_bytes = (size_t)a.n_mlp_params * sizeof(float);
  const bool lds_acc = a.grad_mlp_params && (stage_bytes + param_bytes <= 96 * 1024);
  s.ga.lds_param_accum = lds_acc ? 1 : 0;
  const size_t lds = stage_bytes + (lds_acc ? param_bytes : 0);
  // n_tiles tiles of 64 points, dealt to at most PT_BWD_BLOCKS workgroups of tpb consecutive tiles (tpb is 32-bit like a workgroup count)
  int64_t n_tiles, tpb;
  workgroup_count(s.n_points, 64, n_tiles);
  if (!workgroup_count(n_tiles, PT_BWD_BLOCKS, tpb))
    return set_error(LP_EUNSUPPORTED, "lp_points_backward: %lld points are more than 2^31 tiles per workgroup", (long long)s.n_points);
  s.tiles_per_block = (int32_t)tpb;
  unsigned blocks;
  if (int rc = launch_blocks("lp_points_backward", n_tiles, tpb, blocks)) return rc;
#define LP_LAUNCH_PT_BWD(CAP, ACC)                                                                          \
  do {                                                                                                      \
    hipError_t e = hipFuncSetAttribute((const void*)points_bwd<CAP, ACC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    if (e != hipSuccess) return set_error((int)e, "hipFuncSetAttribute: %s", hipGetErrorString(e));         \
    hipLaunchKernelGGL((points_bwd<CAP, ACC>), dim3(blocks), dim3(64), lds, stream, s);                     \
  } while (0)
  if (total <= 256) {
    if (lds_acc) LP_LAUNCH_PT_BWD(256, true); else LP_LAUNCH_PT_BWD(256, false);
  } else {
    if (lds_acc) LP_LAUNCH_PT_BWD(1024, true); else LP_LAUNCH_PT_BWD(1024, false);
  }
#undef LP_LAUNCH_PT_BWD
  return check_launch("points_bwd");
}

const char* build_info_points() {
  return "{\"forward\": \"one lane per point, one wave per workgroup; fp32 FMA; activations in LDS tiles [width][64] (two, three with "
         "the colour head), weights through wave-uniform scalar loads; no scratch\", \"backward\": \"the shape-generic Renderer backward "
         "without the march: private activation arrays, recompute with wide layers on v_mfma_f32_32x32x2_f32, weight gradients in LDS "
         "accumulators flushed once per workgroup of consecutive 64-point tiles, encoding gradient summed per ray in the wave\"}";
}

}  // namespace lp

// lp_point_grid.hip -- gather and splat of a grid-list at arbitrary 3-D points, without a decoder (C ABI lp_point_gather /
// lp_point_splat / lp_point_normalize / lp_point_grad_points).
//
// The three kernels are the partial derivatives of one bilinear form over points, grids and corners,
//   B(G, P, U) = sum  w_k(q) <G_g[row_k(q)], U[point]>,   q = contract(p) when asked, row_k / w_k = grid_corners<false> (the Renderer's),
// so they are adjoints of each other up to summation order.  A point is element p of the [n_rays, n_pts] array, its batch element
// grid_idx[p / n_pts] (64-bit, clamped), as in lp_points.hip.
//   point_gather_vec   dB/dU, C % 4 == 0: a sub-group of C / 4 consecutive lanes per point, every lane one float4 of the row: a corner
//                      row is one contiguous read of the sub-group and the [point][C] store is contiguous over the whole wave.  Each
//                      lane computes the corner geometry of its point itself (redundantly: no LDS, no barrier).
//   point_gather_lane  dB/dU for any other C: one lane per point, channel loops, the lane's output row as the accumulator.
//   point_splat        dB/dG: one wave per 64 points.  Lane = point writes its corner rows and weights to LDS (three words per corner);
//                      then lanes = CHANNELS: an atomic instruction carries 64 / CW whole rows of C * 4 contiguous bytes (CW = 16 / 32 /
//                      64 lanes per row; the shape of splat_list_wave, lp_generic_mlp.h), U read straight from its [point][C] rows.
//                      Channels 64 .. 127 are a second atomic per row.  Lane 0 of a row also adds w_k to the weight buffer.
//   point_normalize    row /= max(weight, 1e-5), in place, all grids in one launch (blockIdx.y = grid).
//   point_grad_points  dB/dP: one lane per point, point_grad_list + contract_backward (lp_point_grad.h), stored.
// No workspace; nothing but the caller's buffers is written.
#include "lp_host.h"
#include "lp_point_grad.h"
#include "lp_rows.h"

namespace lp {

struct PgArgs {
  LpPointGridArgs a;  // normalised: every grid carries its base pointer
  int64_t n_points;
  int32_t lanes;      // point_gather_vec: lanes per point (C / 4)
};

struct PgPoint {
  Ray ray;
  float x, y, z;  // where the grids are sampled
  bool inside;    // not removed by the out-of-bounds mask
};

LP_DEV PgPoint pg_point(const LpPointGridArgs& a, int64_t p) {
  PgPoint o;
  const int64_t r = p / a.n_pts;
  o.ray = point_ray(a.points, p, clamp_batch(a.grid_idx[r], a.grid.grids[0].B));
  sample_point(o.ray, 0.0f, a.contract_coords != 0, o.x, o.y, o.z);
  o.inside = !(a.mask_out_of_bounds != 0 && !point_in_bounds(o.x, o.y, o.z));
  return o;
}

__global__ void __launch_bounds__(256) point_gather_vec(const PgArgs s) {
  const LpPointGridArgs& a = s.a;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t p = gid / s.lanes;
  if (p >= s.n_points) return;
  const int c0 = 4 * (int)(gid - p * s.lanes);
  const PgPoint pt = pg_point(a, p);
  const int C = a.grid.channels;
  float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (pt.inside) {
    for (int g = 0; g < a.grid.n_grids; ++g) {
      const LpGrid& gd = a.grid.grids[g];
      const Corners cs = grid_corners<false>(gd, pt.ray.b, pt.x, pt.y, pt.z);
      const float* rw = a.row_weight[g];
      float4 v[8];
      float w[8];
      bool ok[8];
      // (a corner outside its grid reads row 0 of the grid's tensor, which exists, with weight 0)
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (k < 4 || cs.n == 8) {
          ok[k] = cs.row[k] >= 0;
          const int64_t row = ok[k] ? cs.row[k] : (int64_t)0;
          v[k] = *reinterpret_cast<const float4*>(gd.data + row * C + c0);
          w[k] = ok[k] ? cs.w[k] : 0.0f;
          if (rw) w[k] = w[k] / fmaxf(rw[row], 1e-5f);
        }
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (k < 4 || cs.n == 8) {
          acc.x = fmaf(w[k], ok[k] ? v[k].x : 0.0f, acc.x);
          acc.y = fmaf(w[k], ok[k] ? v[k].y : 0.0f, acc.y);
          acc.z = fmaf(w[k], ok[k] ? v[k].z : 0.0f, acc.z);
          acc.w = fmaf(w[k], ok[k] ? v[k].w : 0.0f, acc.w);
        }
      }
    }
  }
  reinterpret_cast<float4*>(a.out_features)[gid] = acc;  // (p * C + c0 == 4 * gid)
}

__global__ void __launch_bounds__(256) point_gather_lane(const PgArgs s) {
  const LpPointGridArgs& a = s.a;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= s.n_points) return;
  const PgPoint pt = pg_point(a, p);
  const int C = a.grid.channels;
  float* out = a.out_features + p * C;
  for (int c = 0; c < C; ++c) out[c] = 0.0f;
  if (!pt.inside) return;
  for (int g = 0; g < a.grid.n_grids; ++g) {
    const LpGrid& gd = a.grid.grids[g];
    const Corners cs = grid_corners<false>(gd, pt.ray.b, pt.x, pt.y, pt.z);
    const float* rw = a.row_weight[g];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (k < cs.n && cs.row[k] >= 0) {
        const float* src = gd.data + cs.row[k] * C;
        float w = cs.w[k];
        if (rw) w = w / fmaxf(rw[cs.row[k]], 1e-5f);
        for (int c = 0; c < C; ++c) out[c] = fmaf(w, src[c], out[c]);
      }
    }
  }
}

constexpr int PG_YLD = 24;  // words per point of the corner tile: 8 corners x (row low word, row high word, weight)

template <int CW_LOG>
__global__ void __launch_bounds__(64) point_splat(const PgArgs s) {
  __shared__ float Ys[64 * PG_YLD];
  const LpPointGridArgs& a = s.a;
  const int lane = threadIdx.x;
  const int64_t first = (int64_t)blockIdx.x * 64;
  const int64_t left = s.n_points - first;
  const int rows = left < 64 ? (int)left : 64;  // points of this tile (wave-uniform)
  const bool live = lane < rows;
  const PgPoint pt = pg_point(a, live ? first + lane : 0);  // (a lane past the end looks at point 0 and contributes nothing)
  const bool on = live && pt.inside;
  const int C = a.grid.channels;
  constexpr int PER = 64 >> CW_LOG;  // corner rows per instruction
  const int sub = lane >> CW_LOG, c = lane & ((1 << CW_LOG) - 1);
  float* yr = Ys + lane * PG_YLD;
  for (int g = 0; g < a.grid.n_grids; ++g) {
    const LpGrid& gd = a.grid.grids[g];
    const Corners cs = grid_corners<false>(gd, pt.ray.b, pt.x, pt.y, pt.z);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const bool ok = on && k < cs.n && cs.row[k] >= 0;
      const int64_t row = ok ? cs.row[k] : (int64_t)-1;
      yr[3 * k + 0] = __int_as_float((int)(row & 0xffffffff));
      yr[3 * k + 1] = __int_as_float((int)(row >> 32));
      yr[3 * k + 2] = ok ? cs.w[k] : 0.0f;
    }
    __syncthreads();
    const int nk = (gd.D > 1 && gd.H > 1 && gd.W > 1) ? 8 : 4;  // a property of the grid: wave-uniform
    float* gbase = const_cast<float*>(gd.data);
    float* wbase = a.row_weight[g];
    for (int r0 = 0; r0 < rows; r0 += PER) {
      const int r = r0 + sub;  // < 64: r0 is a multiple of PER below 64
      const bool have = r < rows && c < C;
      const float* u = a.vectors + (first + r) * C;
      const float u0 = have ? u[c] : 0.0f;
      const float u1 = (CW_LOG == 6 && have && 64 + c < C) ? u[64 + c] : 0.0f;
      const float* e = Ys + r * PG_YLD;
      for (int k0 = 0; k0 < nk; k0 += 4) {  // four instructions' operands in flight
        int64_t rowv[4];
        float wv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          rowv[q] = ((int64_t)__float_as_int(e[3 * (k0 + q) + 1]) << 32) | (int64_t)(unsigned)__float_as_int(e[3 * (k0 + q)]);
          wv[q] = e[3 * (k0 + q) + 2];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (have && rowv[q] >= 0) {
            atomic_add_f32(gbase + rowv[q] * C + c, wv[q] * u0);
            if (CW_LOG == 6 && 64 + c < C) atomic_add_f32(gbase + rowv[q] * C + 64 + c, wv[q] * u1);
            if (wbase && c == 0) atomic_add_f32(wbase + rowv[q], wv[q]);
          }
        }
      }
    }
    __syncthreads();
  }
}

struct PgNormArgs {
  float* data[LP_MAX_GRIDS];          // first row of grid g
  const float* weight[LP_MAX_GRIDS];  // weight of that row
  int64_t n_rows[LP_MAX_GRIDS];
  int32_t channels;
};

__global__ void __launch_bounds__(256) point_normalize(const PgNormArgs s) {
  const int g = blockIdx.y;
  const int C = s.channels;
  // (C % 4 == 0: a grid's first row is 16-byte aligned -- row_offset * C * 4 bytes behind an aligned base)
  normalize_rows(s.data[g], s.weight[g], s.n_rows[g], C);
}

__global__ void __launch_bounds__(256) point_grad_points(const PgArgs s) {
  const LpPointGridArgs& a = s.a;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= s.n_points) return;
  const PgPoint pt = pg_point(a, p);
  float gx = 0.0f, gy = 0.0f, gz = 0.0f;
  point_grad_list(a.grid, pt.ray.b, pt.x, pt.y, pt.z, a.mask_out_of_bounds != 0, a.vectors + p * a.grid.channels, gx, gy, gz);
  if (a.contract_coords) contract_backward(pt.ray.ox, pt.ray.oy, pt.ray.oz, gx, gy, gz);
  float* gp = a.grad_points + 3 * p;
  gp[0] = gx;
  gp[1] = gy;
  gp[2] = gz;
}

// ---------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------

int point_gather_launch(const LpPointGridArgs& a, hipStream_t stream) {
  PgArgs s;
  s.a = a;
  s.n_points = a.n_rays * a.n_pts;
  if (s.n_points == 0) return LP_OK;
  const int C = a.grid.channels;
  const bool vec = row_vec(C, {}) == 4;  // (no pointer to look at: lp_api.hip refuses under-aligned ones)
  s.lanes = vec ? C / 4 : 1;
  unsigned blocks;
  if (int rc = launch_blocks("lp_point_gather", s.n_points * s.lanes, 256, blocks)) return rc;
  if (vec)
    hipLaunchKernelGGL(point_gather_vec, dim3(blocks), dim3(256), 0, stream, s);
  else
    hipLaunchKernelGGL(point_gather_lane, dim3(blocks), dim3(256), 0, stream, s);
  return check_launch("point_gather");
}

int point_splat_launch(const LpPointGridArgs& a, hipStream_t stream) {
  PgArgs s;
  s.a = a;
  s.n_points = a.n_rays * a.n_pts;
  s.lanes = 0;
  if (s.n_points == 0) return LP_OK;
  unsigned blocks;
  if (int rc = launch_blocks("lp_point_splat", s.n_points, 64, blocks)) return rc;
  const int C = a.grid.channels;
  if (C <= 16)
    hipLaunchKernelGGL(point_splat<4>, dim3(blocks), dim3(64), 0, stream, s);
  else if (C <= 32)
    hipLaunchKernelGGL(point_splat<5>, dim3(blocks), dim3(64), 0, stream, s);
  else
    hipLaunchKernelGGL(point_splat<6>, dim3(blocks), dim3(64), 0, stream, s);
  return check_launch("point_splat");
}

int point_normalize_launch(const LpPointGridArgs& a, hipStream_t stream) {
  if (a.n_rays * a.n_pts == 0) return LP_OK;  // (the splat added nothing: zero rows stay zero)
  PgNormArgs s{};
  s.channels = a.grid.channels;
  int64_t most = 0;
  for (int g = 0; g < a.grid.n_grids; ++g) {
    const LpGrid& gd = a.grid.grids[g];
    s.data[g] = const_cast<float*>(gd.data) + gd.row_offset * s.channels;
    s.weight[g] = a.row_weight[g] + gd.row_offset;
    s.n_rows[g] = (int64_t)gd.B * gd.D * gd.H * gd.W;
    most = s.n_rows[g] > most ? s.n_rows[g] : most;
  }
  const int64_t per_thread = row_vec(s.channels, {});  // (normalize_rows decides by the channel count alone)
  int64_t blocks = (most * s.channels / per_thread + 255) / 256;
  blocks = blocks < 1 ? 1 : (blocks > 65536 ? 65536 : blocks);  // (grid-stride loop)
  hipLaunchKernelGGL(point_normalize, dim3((unsigned)blocks, (unsigned)a.grid.n_grids), dim3(256), 0, stream, s);
  return check_launch("point_normalize");
}

int point_grad_points_launch(const LpPointGridArgs& a, hipStream_t stream) {
  PgArgs s;
  s.a = a;
  s.n_points = a.n_rays * a.n_pts;
  s.lanes = 1;
  if (s.n_points == 0) return LP_OK;
  unsigned blocks;
  if (int rc = launch_blocks("lp_point_grad_points", s.n_points, 256, blocks)) return rc;
  hipLaunchKernelGGL(point_grad_points, dim3(blocks), dim3(256), 0, stream, s);
  return check_launch("point_grad_points");
}

const char* build_info_point_grid() {
  return "{\"gather\": \"C % 4 == 0: C / 4 lanes per point, one float4 of the row per lane, corner geometry per lane (no LDS); else one "
         "lane per point; no atomics\", \"splat\": \"one wave per 64 points; corner rows and weights through LDS, lanes = channels: 64 / "
         "CW whole rows per atomic instruction (CW = 16 / 32 / 64), a second pass for channels 64 .. 127; weights by lane 0 of a row\", "
         "\"normalize\": \"row /= max(weight, 1e-5) in place, one launch\", \"grad_points\": \"one lane per point, stored\"}";
}

}  // namespace lp

// lp_ray_grid.hip -- weighted splat and gather of a grid-list along rays at caller-given sample depths, without a decoder (DESIGN.md
// 4.21; C ABI lp_ray_grid_splat / lp_ray_grid_gather / lp_ray_grid_grad_samples of include/lightplane_hip_ray_grid.h).
//
// The three kernels are the partial derivatives of
//   T(G, W, F; P) = sum_r sum_s W[r, s] sum_g sum_k  w_k(q_rs) <G_g[row_k(q_rs)], F[r]>,   p_rs = depths[r, s] * directions[r] + origins[r],
// the bilinear form of lp_point_grid.hip with U[r, s] = W[r, s] F[r]: row_k / w_k = grid_corners<false>, q = sample_point (the point
// formation of lp_render_samples.hip: a sample lands in the cell it lands in there), batch element grid_idx[r] clamped.
//   ray_grid_splat         dT/dG: one wavefront = one workgroup per ray, chunks of 64 samples.  Lane = sample writes its corner rows and
//                          the coefficients W w_k to LDS (three words per corner, as point_splat); then lanes = CHANNELS with F[r] in
//                          registers (read once per ray): an atomic instruction carries 64 / CW whole rows of C * 4 contiguous bytes
//                          (CW = 16 / 32 / 64 lanes per row), channels 64 .. 127 a second atomic per row.  Lane 0 of a row also adds the
//                          coefficient to the weight buffer.  A coefficient of exactly 0 (a masked sample, a zero weight, a corner
//                          outside its grid) issues no atomic.
//   ray_grid_gather_vec    dT/dF, C % 4 == 0: one wavefront per ray, C / 4 lanes per sample, every lane one float4 of the row; a lane
//                          adds its samples (every 64 / (C / 4)-th of the ray) in ascending order, then the lanes' sums meet in LDS and
//                          lane c adds channel c over the sub-groups in ascending order: a fixed order, bit-reproducible, no atomics.
//   ray_grid_gather_lane   dT/dF for any other C: per chunk lane = sample leaves rows and coefficients in LDS, then lane c walks the
//                          chunk's samples and corners in ascending order for channels c and 64 + c.
//   ray_grid_grad_samples  dT/dW and dT/d depth: one lane per sample, the corner dot products, point_grad_list + contract_backward
//                          (lp_point_grad.h), stored.
// No workspace, no scratch; nothing but the caller's buffers is written.
#include "lp_host.h"
#include "lp_point_grad.h"
#include "lp_rows.h"
#include "lp_wave.h"

namespace lp {

namespace {

LP_DEV Ray rg_ray(const LpRayGridArgs& a, int64_t r) {
  Ray q;
  load_ray_line(a.origins, a.directions, r, q);
  q.near_t = q.far_t = 0.0f;
  q.b = clamp_batch(a.grid_idx[r], a.grid.grids[0].B);
  return q;
}

constexpr int RG_YLD = 24;  // words per sample of the corner tile: 8 corners x (row low word, row high word, coefficient)

// lane = sample of a chunk: the corner rows of grid `gd` and the coefficients wt * w_k into the lane's entry of the tile (`on` false:
// an entry that contributes nothing)
LP_DEV void rg_stage_corners(const LpGrid& gd, const float* rw, int b, float x, float y, float z, bool on, float wt, float* yr) {
  const Corners cs = grid_corners<false>(gd, b, x, y, z);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const bool ok = on && k < cs.n && cs.row[k] >= 0;
    const int64_t row = ok ? cs.row[k] : (int64_t)-1;
    float cf = ok ? wt * cs.w[k] : 0.0f;
    if (rw && ok) cf = cf / fmaxf(rw[row], 1e-5f);
    yr[3 * k + 0] = __int_as_float((int)(row & 0xffffffff));
    yr[3 * k + 1] = __int_as_float((int)(row >> 32));
    yr[3 * k + 2] = cf;
  }
}

LP_DEV int64_t rg_tile_row(const float* e, int k) {
  return ((int64_t)__float_as_int(e[3 * k + 1]) << 32) | (int64_t)(unsigned)__float_as_int(e[3 * k]);
}

template <int CW_LOG>
__global__ void __launch_bounds__(64) ray_grid_splat(const LpRayGridArgs a) {
  __shared__ float Ys[64 * RG_YLD];
  const int lane = threadIdx.x;
  const int64_t r = blockIdx.x;
  const int S = a.n_samples;
  const int64_t base = r * S;
  const Ray ray = rg_ray(a, r);
  const bool mask = a.mask_out_of_bounds != 0;
  const bool contract = a.contract_coords != 0;
  const int C = a.grid.channels;
  constexpr int PER = 64 >> CW_LOG;  // corner rows per instruction
  const int sub = lane >> CW_LOG, c = lane & ((1 << CW_LOG) - 1);
  // the ray's vector: read once, kept in registers
  const float u0 = c < C ? a.vectors[r * C + c] : 0.0f;
  const float u1 = (CW_LOG == 6 && 64 + c < C) ? a.vectors[r * C + 64 + c] : 0.0f;
  float* yr = Ys + lane * RG_YLD;

  for (int64_t s0 = 0; s0 < S; s0 += 64) {  // (64-bit: the last chunk of a ray of nearly 2^31 samples ends beyond it)
    const int64_t left = S - s0;
    const int rows = left < 64 ? (int)left : 64;  // samples of this chunk (wave-uniform)
    const bool live = lane < rows;
    const int64_t at = base + (live ? s0 + lane : 0);  // (a lane past the end looks at sample 0 and contributes nothing)
    const float dp = a.depths[at];
    const float wt = a.weights[at];
    float x, y, z;
    sample_point(ray, dp, contract, x, y, z);
    const bool on = live && !(mask && !point_in_bounds(x, y, z));
    for (int g = 0; g < a.grid.n_grids; ++g) {
      const LpGrid& gd = a.grid.grids[g];
      rg_stage_corners(gd, nullptr, ray.b, x, y, z, on, wt, yr);
      __syncthreads();
      const int nk = (gd.D > 1 && gd.H > 1 && gd.W > 1) ? 8 : 4;  // a property of the grid: wave-uniform
      float* gbase = const_cast<float*>(gd.data);
      float* wbase = a.row_weight[g];
      for (int i0 = 0; i0 < rows; i0 += PER) {
        const int i = i0 + sub;  // < 64: i0 is a multiple of PER below 64
        const bool have = i < rows && c < C;
        const float* e = Ys + i * RG_YLD;
        for (int k0 = 0; k0 < nk; k0 += 4) {  // four instructions' operands in flight
          int64_t rowv[4];
          float wv[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            rowv[q] = rg_tile_row(e, k0 + q);
            wv[q] = e[3 * (k0 + q) + 2];
          }
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (have && rowv[q] >= 0 && wv[q] != 0.0f) {
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
}

struct RgGatherArgs {
  LpRayGridArgs a;
  int32_t lanes;  // ray_grid_gather_vec: lanes per sample (C / 4)
  int32_t per;    // ... and samples per pass (64 / lanes)
};

__global__ void __launch_bounds__(64) ray_grid_gather_vec(const RgGatherArgs s) {
  __shared__ float4 Ps[64];
  const LpRayGridArgs& a = s.a;
  const int lane = threadIdx.x;
  const int64_t r = blockIdx.x;
  const int S = a.n_samples;
  const int64_t base = r * S;
  const Ray ray = rg_ray(a, r);
  const bool mask = a.mask_out_of_bounds != 0;
  const bool contract = a.contract_coords != 0;
  const int C = a.grid.channels;
  const int sub = lane / s.lanes;             // the lane's sample of a pass
  const int c0 = 4 * (lane - sub * s.lanes);  // its four channels
  const bool active = sub < s.per;            // (64 % lanes != 0: the last lanes idle)
  float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  for (int64_t sm = sub; active && sm < S; sm += s.per) {  // ascending: a fixed order per lane
    const float dp = a.depths[base + sm];
    const float wt = a.weights[base + sm];
    float x, y, z;
    sample_point(ray, dp, contract, x, y, z);
    if (mask && !point_in_bounds(x, y, z)) continue;
    for (int g = 0; g < a.grid.n_grids; ++g) {
      const LpGrid& gd = a.grid.grids[g];
      const Corners cs = grid_corners<false>(gd, ray.b, x, y, z);
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
          w[k] = ok[k] ? wt * cs.w[k] : 0.0f;
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
  Ps[lane] = acc;  // (lane = sub * lanes + c0 / 4: sub-group `sub` holds its C floats at word sub * C)
  __syncthreads();
  const float* tile = reinterpret_cast<const float*>(Ps);
  for (int ch = lane; ch < C; ch += 64) {
    float sum = 0.0f;
    for (int j = 0; j < s.per; ++j) sum += tile[j * C + ch];  // sub-groups in ascending order
    a.out_features[r * C + ch] = sum;
  }
}

__global__ void __launch_bounds__(64) ray_grid_gather_lane(const LpRayGridArgs a) {
  __shared__ float Ys[64 * RG_YLD];
  const int lane = threadIdx.x;
  const int64_t r = blockIdx.x;
  const int S = a.n_samples;
  const int64_t base = r * S;
  const Ray ray = rg_ray(a, r);
  const bool mask = a.mask_out_of_bounds != 0;
  const bool contract = a.contract_coords != 0;
  const int C = a.grid.channels;
  float* yr = Ys + lane * RG_YLD;
  float acc0 = 0.0f, acc1 = 0.0f;  // channels lane and 64 + lane
  for (int64_t s0 = 0; s0 < S; s0 += 64) {
    const int64_t left = S - s0;
    const int rows = left < 64 ? (int)left : 64;
    const bool live = lane < rows;
    const int64_t at = base + (live ? s0 + lane : 0);
    const float dp = a.depths[at];
    const float wt = a.weights[at];
    float x, y, z;
    sample_point(ray, dp, contract, x, y, z);
    const bool on = live && !(mask && !point_in_bounds(x, y, z));
    for (int g = 0; g < a.grid.n_grids; ++g) {
      const LpGrid& gd = a.grid.grids[g];
      rg_stage_corners(gd, a.row_weight[g], ray.b, x, y, z, on, wt, yr);
      __syncthreads();
      const int nk = (gd.D > 1 && gd.H > 1 && gd.W > 1) ? 8 : 4;
      for (int i = 0; i < rows; ++i) {  // samples, then corners, in ascending order: a fixed order
        const float* e = Ys + i * RG_YLD;
        for (int k = 0; k < nk; ++k) {
          const int64_t row = rg_tile_row(e, k);
          const float w = e[3 * k + 2];
          if (row >= 0) {  // (wave-uniform: every lane reads the same entry)
            const float* src = gd.data + row * C;
            if (lane < C) acc0 = fmaf(w, src[lane], acc0);
            if (64 + lane < C) acc1 = fmaf(w, src[64 + lane], acc1);
          }
        }
      }
      __syncthreads();
    }
  }
  if (lane < C) a.out_features[r * C + lane] = acc0;
  if (64 + lane < C) a.out_features[r * C + 64 + lane] = acc1;
}

__global__ void __launch_bounds__(256) ray_grid_grad_samples(const LpRayGridArgs a) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int S = a.n_samples;
  if (p >= a.n_rays * S) return;
  const int64_t r = p / S;
  const Ray ray = rg_ray(a, r);
  const bool mask = a.mask_out_of_bounds != 0;
  const int C = a.grid.channels;
  const float dp = a.depths[p];
  const float* f = a.vectors + r * C;
  float x, y, z;
  sample_point(ray, dp, a.contract_coords != 0, x, y, z);
  if (a.grad_weights) {
    float val = 0.0f;
    if (!(mask && !point_in_bounds(x, y, z))) {
      for (int g = 0; g < a.grid.n_grids; ++g) {
        const LpGrid& gd = a.grid.grids[g];
        const Corners cs = grid_corners<false>(gd, ray.b, x, y, z);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          if (k < cs.n && cs.row[k] >= 0) {
            const float* src = gd.data + cs.row[k] * C;
            float dot = 0.0f;
            for (int c = 0; c < C; ++c) dot = fmaf(src[c], f[c], dot);
            val = fmaf(cs.w[k], dot, val);
          }
        }
      }
    }
    a.grad_weights[p] = val;
  }
  if (a.grad_depths) {
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
    point_grad_list(a.grid, ray.b, x, y, z, mask, f, gx, gy, gz);
    if (a.contract_coords) {
      float px, py, pz;  // the point before the contraction
      sample_point(ray, dp, false, px, py, pz);
      contract_backward(px, py, pz, gx, gy, gz);
    }
    a.grad_depths[p] = a.weights[p] * (gx * ray.dx + gy * ray.dy + gz * ray.dz);
  }
}

}  // namespace

// `a` normalised and checked by lp_api.hip: n_rays > 0, n_samples > 0, n_rays * n_samples < 2^31 (one workgroup per ray: n_rays is a
// legal grid dimension)
int ray_grid_splat_launch(const LpRayGridArgs& a, hipStream_t stream) {
  unsigned blocks;
  if (int rc = launch_blocks("lp_ray_grid_splat", a.n_rays, 1, blocks)) return rc;
  const int C = a.grid.channels;
  if (C <= 16)
    hipLaunchKernelGGL(ray_grid_splat<4>, dim3(blocks), dim3(64), 0, stream, a);
  else if (C <= 32)
    hipLaunchKernelGGL(ray_grid_splat<5>, dim3(blocks), dim3(64), 0, stream, a);
  else
    hipLaunchKernelGGL(ray_grid_splat<6>, dim3(blocks), dim3(64), 0, stream, a);
  return check_launch("ray_grid_splat");
}

int ray_grid_gather_launch(const LpRayGridArgs& a, hipStream_t stream) {
  unsigned blocks;
  if (int rc = launch_blocks("lp_ray_grid_gather", a.n_rays, 1, blocks)) return rc;
  const int C = a.grid.channels;
  if (row_vec(C, {}) == 4) {  // (no pointer to look at: lp_api.hip refuses under-aligned ones)
    RgGatherArgs s;
    s.a = a;
    s.lanes = C / 4;
    s.per = 64 / s.lanes;
    hipLaunchKernelGGL(ray_grid_gather_vec, dim3(blocks), dim3(64), 0, stream, s);
  } else {
    hipLaunchKernelGGL(ray_grid_gather_lane, dim3(blocks), dim3(64), 0, stream, a);
  }
  return check_launch("ray_grid_gather");
}

int ray_grid_grad_samples_launch(const LpRayGridArgs& a, hipStream_t stream) {
  unsigned blocks;
  if (int rc = launch_blocks("lp_ray_grid_grad_samples", a.n_rays * a.n_samples, 256, blocks)) return rc;
  hipLaunchKernelGGL(ray_grid_grad_samples, dim3(blocks), dim3(256), 0, stream, a);
  return check_launch("ray_grid_grad_samples");
}

}  // namespace lp

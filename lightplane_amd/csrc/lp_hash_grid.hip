// lp_hash_grid.hip -- multiresolution hash-grid encoding of 3-D points, forward and both gradients (C ABI
// lp_hash_grid_forward / lp_hash_grid_backward_table / lp_hash_grid_backward_points, include/lightplane_hip_hash_grid.h, which holds the
// definition).  The layout (resolution, offset, size, dense / hashed of every level) is the caller's: the kernels read it from the
// argument block with a wave-uniform index and compute no growth factor.  fp32 coordinates limit a level's interpolation weights to
// about N_l * 2^-24 cells.
//   hash_encode_fwd<F>         work item (point, level): lane = point in the flattened [n_rays * n_pts] order, blockIdx.y = LEVEL, the slow
//                              index of the launch -- the workgroups in flight at one time read one level's table (a 2^19 x 2 level is
//                              4 MB, 16 of them are not an L2's worth).  The point's geometry is formed once, the 8 corner loads of 4 F
//                              bytes are issued before the first use, the F results leave as one store.  No LDS, no atomics.
//   hash_encode_bwd_table<F>   the same mapping; a lane adds w_k dY to its 8 entries with fp32 atomics.  Consecutive lanes are consecutive
//                              samples of a ray, and on the coarse levels they share a cell: a lane whose (b, cell) differs from the
//                              previous lane's is a run HEAD (lane 0 always).  A wave without a non-head lane (one ballot) issues its
//                              atomics lane by lane; otherwise the 8 F products are summed over every run with a segmented suffix scan
//                              (shuffles, fixed order) and only heads issue atomics.  The branch is wave-uniform; runs end with the wave.
//   hash_encode_bwd_points<F>  lane = point, loop over the levels: the upstream row is read 16 bytes at a time, the derivative of the
//                              weights meets <table row, dY of the level> N_l / 2, then contract_backward; three stores, no atomics.
// 64-bit entry offsets throughout; no workspace; nothing but the caller's buffers is written.
#include "lp_hash_levels.h"

namespace lp {

struct HgArgs {
  LpHashGridArgs a;
  int64_t n_points;
};

template <int F>
__global__ void __launch_bounds__(256) hash_encode_fwd(const HgArgs s) {
  const LpHashGridArgs& a = s.a;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= s.n_points) return;
  const int l = blockIdx.y;
  const HgLevel lv = hg_level(a, l);
  const HgPoint pt = hg_point(a, p);
  const HgRow<F> acc = hg_interp<F>(a, pt, lv);
  hg_store<F>(a.out_features + p * ((int64_t)a.n_levels * F) + l * F, acc);
}

template <int F>
__global__ void __launch_bounds__(256) hash_encode_bwd_table(const HgArgs s) {
  const LpHashGridArgs& a = s.a;
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = p < s.n_points;  // (a lane past the end looks at point 0, contributes nothing and takes part in the shuffles)
  const int l = blockIdx.y;
  const HgLevel lv = hg_level(a, l);
  const HgPoint pt = hg_point(a, live ? p : 0);
  const bool on = live && pt.inside;
  const HgCell cell = hg_cell(pt, lv);
  HgRow<F> dy;
#pragma unroll
  for (int c = 0; c < F; ++c) dy.v[c] = 0.0f;
  if (on) dy = hg_load<F>(a.grad_features + p * ((int64_t)a.n_levels * F) + l * F);

  const HgRun run = hg_run(cell, pt.ray.b, on, lane);
  hg_table_grad<F>(a.grad_table + hg_base(a, pt.ray.b, lv, F), cell, lv, dy, on, run);
}

template <int F>
__global__ void __launch_bounds__(256) hash_encode_bwd_points(const HgArgs s) {
  const LpHashGridArgs& a = s.a;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= s.n_points) return;
  const HgPoint pt = hg_point(a, p);
  float gx = 0.0f, gy = 0.0f, gz = 0.0f;
  if (pt.inside) {
    constexpr int GF = F < 4 ? 4 : F;  // floats of the upstream row per step: whole 16-byte reads
    constexpr int PER = GF / F;        // levels per step
    const int L = a.n_levels, LF = L * F;
    const float* row = a.grad_features + p * (int64_t)LF;
    const bool vec = (LF & 3) == 0;  // (the rows are 16-byte aligned; otherwise float by float)
    for (int l0 = 0; l0 < L; l0 += PER) {
      float d[GF];
      if (vec) {
#pragma unroll
        for (int j = 0; j < GF / 4; ++j) {
          const float4 t = reinterpret_cast<const float4*>(row + l0 * F)[j];
          d[4 * j + 0] = t.x; d[4 * j + 1] = t.y; d[4 * j + 2] = t.z; d[4 * j + 3] = t.w;
        }
      } else {
#pragma unroll
        for (int j = 0; j < GF; ++j) d[j] = l0 * F + j < LF ? row[l0 * F + j] : 0.0f;
      }
#pragma unroll
      for (int li = 0; li < PER; ++li) {
        const int l = l0 + li;
        if (l < L) {  // wave-uniform
          hg_point_grad<F>(a, pt, hg_level(a, l), d + li * F, gx, gy, gz);
        }
      }
    }
    if (a.contract_coords) contract_backward(pt.ray.ox, pt.ray.oy, pt.ray.oz, gx, gy, gz);
  }
  float* gp = a.grad_points + 3 * p;
  gp[0] = gx;
  gp[1] = gy;
  gp[2] = gz;
}

// ---------------------------------------------------------------------------------------------------------------------------
// host side (`a` checked by lp_api.hip; n_rays * n_pts > 0)
// ---------------------------------------------------------------------------------------------------------------------------

#define LP_HG_LAUNCH(kernel, grid)                                                          \
  switch (a.features_per_level) {                                                           \
    case 1: hipLaunchKernelGGL(kernel<1>, grid, dim3(256), 0, stream, s); break;            \
    case 2: hipLaunchKernelGGL(kernel<2>, grid, dim3(256), 0, stream, s); break;            \
    case 4: hipLaunchKernelGGL(kernel<4>, grid, dim3(256), 0, stream, s); break;            \
    default: hipLaunchKernelGGL(kernel<8>, grid, dim3(256), 0, stream, s); break;           \
  }

static int hash_grid_launch(const char* what, const LpHashGridArgs& a, int mode, hipStream_t stream) {
  HgArgs s;
  s.a = a;
  s.n_points = a.n_rays * a.n_pts;
  unsigned blocks;
  if (int rc = launch_blocks(what, s.n_points, 256, blocks)) return rc;
  const dim3 per_level(blocks, (unsigned)a.n_levels);  // x runs fastest: a level's workgroups are dispatched together
  if (mode == 0) {
    LP_HG_LAUNCH(hash_encode_fwd, per_level)
  } else if (mode == 1) {
    LP_HG_LAUNCH(hash_encode_bwd_table, per_level)
  } else {
    LP_HG_LAUNCH(hash_encode_bwd_points, dim3(blocks))
  }
  return check_launch(what);
}

int hash_grid_forward_launch(const LpHashGridArgs& a, hipStream_t stream) { return hash_grid_launch("lp_hash_grid_forward", a, 0, stream); }
int hash_grid_backward_table_launch(const LpHashGridArgs& a, hipStream_t stream) {
  return hash_grid_launch("lp_hash_grid_backward_table", a, 1, stream);
}
int hash_grid_backward_points_launch(const LpHashGridArgs& a, hipStream_t stream) {
  return hash_grid_launch("lp_hash_grid_backward_points", a, 2, stream);
}

}  // namespace lp

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
#include "lp_host.h"
#include "lp_point_grad.h"
#include "lp_wave.h"

namespace lp {

struct HgArgs {
  LpHashGridArgs a;
  int64_t n_points;
};

// what a level is, read once per wave from the argument block
struct HgLevel {
  float n;        // N_l
  float half;     // N_l / 2 (exact)
  uint32_t side;  // S_l = N_l + 1
  uint32_t mask;  // size - 1 of a hashed level
  bool hashed;
  int64_t offset;
};

LP_DEV HgLevel hg_level(const LpHashGridArgs& a, int l) {
  HgLevel v;
  const int n = a.resolution[l];
  v.n = (float)n;
  v.half = 0.5f * v.n;
  v.side = (uint32_t)n + 1u;
  v.mask = (uint32_t)a.size[l] - 1u;
  v.hashed = a.hashed[l] != 0;
  v.offset = a.offset[l];
  return v;
}

struct HgPoint {
  Ray ray;        // (ox, oy, oz): the point as given
  float x, y, z;  // where the levels are sampled
  bool inside;    // not removed by the out-of-bounds mask
};

LP_DEV HgPoint hg_point(const LpHashGridArgs& a, int64_t p) {
  HgPoint o;
  const int64_t r = p / a.n_pts;
  o.ray = point_ray(a.points, p, clamp_batch(a.grid_idx[r], a.batch));
  sample_point(o.ray, 0.0f, a.contract_coords != 0, o.x, o.y, o.z);
  o.inside = !(a.mask_out_of_bounds != 0 && !point_in_bounds(o.x, o.y, o.z));
  return o;
}

struct HgAxis {
  uint32_t i;  // base vertex, 0 .. N_l - 1
  float f;     // weight of vertex i + 1
  bool free;   // x was not clamped: the axis carries a gradient
};

// x = q N / 2 + N / 2 in one rounding; a coordinate that is not a number lands on vertex 0
LP_DEV HgAxis hg_axis(float q, const HgLevel& lv) {
  const float t = fmaf(q, lv.half, lv.half);
  const float x = fminf(fmaxf(t, 0.0f), lv.n);
  const float fl = fminf(floorf(x), lv.n - 1.0f);
  HgAxis o;
  o.i = (uint32_t)(int)fl;
  o.f = x - fl;
  o.free = t >= 0.0f && t <= lv.n;
  return o;
}

struct HgCell {
  HgAxis x, y, z;
};

LP_DEV HgCell hg_cell(const HgPoint& pt, const HgLevel& lv) { return {hg_axis(pt.x, lv), hg_axis(pt.y, lv), hg_axis(pt.z, lv)}; }

// entry of corner k (bit 0: x, bit 1: y, bit 2: z) inside its level; lv.hashed is wave-uniform
LP_DEV int64_t hg_entry(const HgCell& c, const HgLevel& lv, int k) {
  const uint32_t ix = c.x.i + (uint32_t)(k & 1), iy = c.y.i + (uint32_t)((k >> 1) & 1), iz = c.z.i + (uint32_t)((k >> 2) & 1);
  const uint32_t e = lv.hashed ? ((ix ^ (iy * 2654435761u) ^ (iz * 805459861u)) & lv.mask) : ix + lv.side * (iy + lv.side * iz);
  return (int64_t)e;
}

LP_DEV float hg_pick(const HgAxis& a, int hi) { return hi ? a.f : 1.0f - a.f; }
LP_DEV float hg_weight(const HgCell& c, int k) { return hg_pick(c.x, k & 1) * hg_pick(c.y, (k >> 1) & 1) * hg_pick(c.z, (k >> 2) & 1); }

// F consecutive floats as one access of 4 F bytes (two of 16 for F = 8); `p` is aligned to that many bytes
template <int F>
struct HgRow {
  float v[F];
};

template <int F>
LP_DEV HgRow<F> hg_load(const float* p) {
  HgRow<F> r;
  if constexpr (F == 1) {
    r.v[0] = p[0];
  } else if constexpr (F == 2) {
    const float2 t = *reinterpret_cast<const float2*>(p);
    r.v[0] = t.x; r.v[1] = t.y;
  } else {
#pragma unroll
    for (int j = 0; j < F / 4; ++j) {
      const float4 t = reinterpret_cast<const float4*>(p)[j];
      r.v[4 * j + 0] = t.x; r.v[4 * j + 1] = t.y; r.v[4 * j + 2] = t.z; r.v[4 * j + 3] = t.w;
    }
  }
  return r;
}

template <int F>
LP_DEV void hg_store(float* p, const HgRow<F>& r) {
  if constexpr (F == 1) {
    p[0] = r.v[0];
  } else if constexpr (F == 2) {
    *reinterpret_cast<float2*>(p) = make_float2(r.v[0], r.v[1]);
  } else {
#pragma unroll
    for (int j = 0; j < F / 4; ++j)
      reinterpret_cast<float4*>(p)[j] = make_float4(r.v[4 * j + 0], r.v[4 * j + 1], r.v[4 * j + 2], r.v[4 * j + 3]);
  }
}

// first float of level `lv` of batch element b
LP_DEV int64_t hg_base(const LpHashGridArgs& a, int b, const HgLevel& lv, int F) { return ((int64_t)b * a.entries + lv.offset) * F; }

template <int F>
__global__ void __launch_bounds__(256) hash_encode_fwd(const HgArgs s) {
  const LpHashGridArgs& a = s.a;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= s.n_points) return;
  const int l = blockIdx.y;
  const HgLevel lv = hg_level(a, l);
  const HgPoint pt = hg_point(a, p);
  HgRow<F> acc;
#pragma unroll
  for (int c = 0; c < F; ++c) acc.v[c] = 0.0f;
  if (pt.inside) {
    const HgCell cell = hg_cell(pt, lv);
    const float* level = a.table + hg_base(a, pt.ray.b, lv, F);
    HgRow<F> v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = hg_load<F>(level + hg_entry(cell, lv, k) * F);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float w = hg_weight(cell, k);
#pragma unroll
      for (int c = 0; c < F; ++c) acc.v[c] = fmaf(w, v[k].v[c], acc.v[c]);
    }
  }
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

  // run heads: (b, cell) differs from the previous lane's, or one of the two adds nothing
  const uint32_t kxy = cell.x.i | (cell.y.i << 16), kz = cell.z.i;  // (vertex indices stay below 2^16)
  const bool same = __shfl_up(kxy, 1, 64) == kxy && __shfl_up(kz, 1, 64) == kz && __shfl_up(pt.ray.b, 1, 64) == pt.ray.b &&
                    __shfl_up((int)on, 1, 64) != 0;
  const bool head = lane == 0 || !on || !same;
  const uint64_t heads = __ballot(head);
  const bool merge = heads != ~(uint64_t)0;  // wave-uniform
  // lanes behind this one in its run: up to the next head, or to the end of the wave
  const uint64_t rest = lane < 63 ? heads >> (lane + 1) : (uint64_t)0;
  const int follow = rest != 0 ? __builtin_ctzll(rest) : 63 - lane;

  float* level = a.grad_table + hg_base(a, pt.ray.b, lv, F);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float w = hg_weight(cell, k);
    float v[F];
#pragma unroll
    for (int c = 0; c < F; ++c) v[c] = w * dy.v[c];
    if (merge) {  // segmented suffix sum: afterwards a head holds its run's total
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
        for (int c = 0; c < F; ++c) {
          const float y = __shfl_down(v[c], d, 64);
          if (d <= follow) v[c] += y;
        }
      }
    }
    if (on && head) {
      float* dst = level + hg_entry(cell, lv, k) * F;
#pragma unroll
      for (int c = 0; c < F; ++c) atomic_add_f32(dst + c, v[c]);
    }
  }
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
          const HgLevel lv = hg_level(a, l);
          const HgCell cell = hg_cell(pt, lv);
          const float* level = a.table + hg_base(a, pt.ray.b, lv, F);
          HgRow<F> v[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) v[k] = hg_load<F>(level + hg_entry(cell, lv, k) * F);
          const float hx = cell.x.free ? lv.half : 0.0f, hy = cell.y.free ? lv.half : 0.0f, hz = cell.z.free ? lv.half : 0.0f;
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            float dot = 0.0f;
#pragma unroll
            for (int c = 0; c < F; ++c) dot = fmaf(v[k].v[c], d[li * F + c], dot);
            const int ux = k & 1, uy = (k >> 1) & 1, uz = (k >> 2) & 1;
            const float wx = hg_pick(cell.x, ux), wy = hg_pick(cell.y, uy), wz = hg_pick(cell.z, uz);
            gx = fmaf(dot, (ux ? hx : -hx) * wy * wz, gx);
            gy = fmaf(dot, wx * (uy ? hy : -hy) * wz, gy);
            gz = fmaf(dot, wx * wy * (uz ? hz : -hz), gz);
          }
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

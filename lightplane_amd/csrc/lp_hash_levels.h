// lp_hash_levels.h -- a multiresolution hash grid as a lane sees it: level constants, the point's geometry, cell, entries, weights and
// rows, one level's interpolation and point gradient, and the run merge of the table gradient.  Shared by the stand-alone encoding
// (lp_hash_grid.hip), the decoder on a hash grid at points (lp_hash_points.hip) and the render along rays (lp_hash_render.hip), which
// carry their layout as an LpHashGridArgs too.
// (include/lightplane_hip_hash_grid.h holds the definition.)
#pragma once
#include "lp_host.h"
#include "lp_point_grad.h"
#include "lp_wave.h"

namespace lp {

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

// the same for a point formed in registers: (x, y, z) = sample_point(ray, depth, contract), `ray` with its batch element clamped
// (lp_hash_render.hip: one ray per wave, so ray.b and with it every level's table base is wave-uniform)
LP_DEV HgPoint hg_point_at(const Ray& ray, float x, float y, float z, bool mask_out_of_bounds) {
  HgPoint o;
  o.ray = ray;
  o.x = x, o.y = y, o.z = z;
  o.inside = !(mask_out_of_bounds && !point_in_bounds(x, y, z));
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

// the F features of one level at the point: the 8 corner loads are issued before the first use; all zero for a masked point
template <int F>
LP_DEV HgRow<F> hg_interp(const LpHashGridArgs& a, const HgPoint& pt, const HgLevel& lv) {
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
  return acc;
}

// the F features of level `lv` into out[c * STRIDE], c < F; F wave-uniform
template <int F, int STRIDE>
LP_DEV void hp_level_f(const LpHashGridArgs& g, const HgPoint& pt, const HgLevel& lv, float* out) {
  const HgRow<F> v = hg_interp<F>(g, pt, lv);
#pragma unroll
  for (int c = 0; c < F; ++c) out[c * STRIDE] = v.v[c];
}

// every level's features into out[(l F + c) * STRIDE]: point-major, F dispatched by a wave-uniform switch
template <int STRIDE>
LP_DEV void hp_features(const LpHashGridArgs& g, const HgPoint& pt, float* out) {
  const int F = g.features_per_level;
  for (int l = 0; l < g.n_levels; ++l) {
    const HgLevel lv = hg_level(g, l);
    float* o = out + l * F * STRIDE;
    switch (F) {
      case 1: hp_level_f<1, STRIDE>(g, pt, lv, o); break;
      case 2: hp_level_f<2, STRIDE>(g, pt, lv, o); break;
      case 4: hp_level_f<4, STRIDE>(g, pt, lv, o); break;
      default: hp_level_f<8, STRIDE>(g, pt, lv, o); break;
    }
  }
}

// (gx, gy, gz) += sum over the corners of (d w_k / d x) <table row, d> N_l / 2, d the gradient of the level's F features: 0 on a
// clamped axis.  For a point that is `inside`.
template <int F>
LP_DEV void hg_point_grad(const LpHashGridArgs& a, const HgPoint& pt, const HgLevel& lv, const float* d, float& gx, float& gy, float& gz) {
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
    for (int c = 0; c < F; ++c) dot = fmaf(v[k].v[c], d[c], dot);
    const int ux = k & 1, uy = (k >> 1) & 1, uz = (k >> 2) & 1;
    const float wx = hg_pick(cell.x, ux), wy = hg_pick(cell.y, uy), wz = hg_pick(cell.z, uz);
    gx = fmaf(dot, (ux ? hx : -hx) * wy * wz, gx);
    gy = fmaf(dot, wx * (uy ? hy : -hy) * wz, gy);
    gz = fmaf(dot, wx * wy * (uz ? hz : -hz), gz);
  }
}

// Runs of the table gradient.  Consecutive lanes are consecutive samples of a ray, and on the coarse levels they share a cell: a lane
// whose (b, cell) differs from the previous lane's, or that adds nothing (`on` false), is a run HEAD (lane 0 always); runs end with the
// wave.  Every lane of the wave calls this.
struct HgRun {
  bool head;
  bool merge;  // wave-uniform: some lane is not a head
  int follow;  // lanes behind this one in its run: up to the next head, or to the end of the wave
};

// `same`: this lane continues the run of the lane before it
LP_DEV HgRun hg_run_of(bool same, bool on, int lane) {
  HgRun r;
  r.head = lane == 0 || !on || !same;
  const uint64_t heads = __ballot(r.head);
  r.merge = heads != ~(uint64_t)0;
  const uint64_t rest = lane < 63 ? heads >> (lane + 1) : (uint64_t)0;
  r.follow = rest != 0 ? __builtin_ctzll(rest) : 63 - lane;
  return r;
}

LP_DEV HgRun hg_run(const HgCell& cell, int b, bool on, int lane) {
  const uint32_t kxy = cell.x.i | (cell.y.i << 16), kz = cell.z.i;  // (vertex indices stay below 2^16)
  const bool same = __shfl_up(kxy, 1, 64) == kxy && __shfl_up(kz, 1, 64) == kz && __shfl_up(b, 1, 64) == b &&
                    __shfl_up((int)on, 1, 64) != 0;
  return hg_run_of(same, on, lane);
}

// a wave that holds ONE ray (lp_hash_render.hip): the lanes share the batch element, so there is no batch comparison; the three
// shuffles are made by every lane
LP_DEV HgRun hg_run_ray(const HgCell& cell, bool on, int lane) {
  const uint32_t kxy = cell.x.i | (cell.y.i << 16), kz = cell.z.i;
  const uint32_t pxy = __shfl_up(kxy, 1, 64), pz = __shfl_up(kz, 1, 64);
  const int pon = __shfl_up((int)on, 1, 64);
  return hg_run_of(pxy == kxy && pz == kz && pon != 0, on, lane);
}

// w_k d of this lane for the 8 corners of its cell go to `level` (the level's first float in the gradient table) with fp32 atomics.
// A wave without a run of two issues them lane by lane; otherwise the products are summed over every run with a segmented suffix scan
// (shuffles, fixed order: afterwards a head holds its run's total) and only heads issue atomics.  The branch is wave-uniform; every
// lane of the wave calls this, `d` all zero for a lane that is not `on`.
template <int F>
LP_DEV void hg_table_grad(float* level, const HgCell& cell, const HgLevel& lv, const HgRow<F>& d, bool on, const HgRun& run) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float w = hg_weight(cell, k);
    float v[F];
#pragma unroll
    for (int c = 0; c < F; ++c) v[c] = w * d.v[c];
    if (run.merge) {
#pragma unroll
      for (int s = 1; s < 64; s <<= 1) {
#pragma unroll
        for (int c = 0; c < F; ++c) {
          const float y = __shfl_down(v[c], s, 64);
          if (s <= run.follow) v[c] += y;
        }
      }
    }
    if (on && run.head) {
      float* dst = level + hg_entry(cell, lv, k) * F;
#pragma unroll
      for (int c = 0; c < F; ++c) atomic_add_f32(dst + c, v[c]);
    }
  }
}

}  // namespace lp

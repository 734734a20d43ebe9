// lp_kplanes_planes.h -- the device helpers of the space-time plane encoding that both of its units need: the stand-alone encoding
// (lp_kplanes.hip) and the decoder fused on it at points (lp_kplanes_points.hip).  The axis map, a point's geometry, its cell on a
// scale, the base row of a plane, the plane / axis tables KP_U / KP_V, the folds of four vertices and the flush of a plane's four
// vertex sums.  include/lightplane_hip_kplanes.h holds the definition; the arithmetic and its order are the same in every caller.
#pragma once
#include "lp_host.h"
#include "lp_point_grad.h"
#include "lp_wave.h"

namespace lp {

// plane j of a scale lies over the axes (KP_U[j], KP_V[j]) of (x, y, z, t); the first is always spatial
#define KP_U(j) ((j) == 0 || (j) == 1 || (j) == 3 ? 0 : ((j) == 2 || (j) == 4 ? 1 : 2))
#define KP_V(j) ((j) == 0 ? 1 : ((j) == 1 || (j) == 2 ? 2 : 3))

struct KpAxis {
  int i;      // base vertex, 0 .. n - 2
  float f;    // weight of vertex i + 1
  bool free;  // x was not clamped: the axis carries a gradient
};

// x = q (n - 1) / 2 + (n - 1) / 2 in one rounding; a coordinate that is not a number lands on vertex 0
LP_DEV KpAxis kp_axis(float q, int n) {
  const float top = (float)(n - 1), half = 0.5f * top;
  const float t = fmaf(q, half, half);
  const float x = fminf(fmaxf(t, 0.0f), top);
  const float fl = fminf(floorf(x), top - 1.0f);
  KpAxis o;
  o.i = (int)fl;
  o.f = x - fl;
  o.free = t >= 0.0f && t <= top;
  return o;
}

struct KpPoint {
  Ray ray;        // (ox, oy, oz): the point as given
  float x, y, z;  // where the planes are sampled
  float t;        // the timestamp (0 for a static layout)
  bool inside;    // not removed by the out-of-bounds mask
};

// point p < n_points < 2^31 of row p / n_pts
template <int P>
LP_DEV KpPoint kp_point(const LpKPlanesArgs& a, int64_t p) {
  KpPoint o;
  const uint32_t r = (uint32_t)p / (uint32_t)a.n_pts;
  o.ray = point_ray(a.points, p, clamp_batch(a.grid_idx[r], a.batch));
  sample_point(o.ray, 0.0f, a.contract_coords != 0, o.x, o.y, o.z);
  o.inside = !(a.mask_out_of_bounds != 0 && !point_in_bounds(o.x, o.y, o.z));
  o.t = 0.0f;
  if constexpr (P == 6) o.t = a.times[a.time_per_point ? p : (int64_t)r];
  return o;
}

// the cell of a point on the four axes of one scale
struct KpCell {
  KpAxis ax[4];
  int n;  // n_s: the row stride of the second axis on every plane
};

template <int P>
LP_DEV KpCell kp_cell(const LpKPlanesArgs& a, const KpPoint& pt, int s) {
  KpCell c;
  c.n = a.spatial[s];
  c.ax[0] = kp_axis(pt.x, c.n);
  c.ax[1] = kp_axis(pt.y, c.n);
  c.ax[2] = kp_axis(pt.z, c.n);
  if constexpr (P == 6) c.ax[3] = kp_axis(pt.t, a.temporal[s]);
  else c.ax[3] = KpAxis{0, 0.0f, false};
  return c;
}

// row of the base vertex of plane j inside the [batch * rows] rows of the tensor
LP_DEV int64_t kp_base_row(const LpKPlanesArgs& a, const KpCell& c, int b, int s, int j) {
  return (int64_t)b * a.rows + a.offset[s][j] + (int64_t)c.ax[KP_U(j)].i + (int64_t)c.n * (int64_t)c.ax[KP_V(j)].i;
}

LP_DEV float4 kp_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
LP_DEV float4 kp_mul(const float4& x, const float4& y) { return make_float4(x.x * y.x, x.y * y.y, x.z * y.z, x.w * y.w); }
LP_DEV float kp_dot(const float4& x, const float4& y) { return fmaf(x.w, y.w, fmaf(x.z, y.z, fmaf(x.y, y.y, x.x * y.x))); }
// w0 t0 + w1 t1 + w2 t2 + w3 t3, in that order
LP_DEV float4 kp_fold(const float4* t, float w0, float w1, float w2, float w3) {
  float4 v;
  v.x = fmaf(w3, t[3].x, fmaf(w2, t[2].x, fmaf(w1, t[1].x, w0 * t[0].x)));
  v.y = fmaf(w3, t[3].y, fmaf(w2, t[2].y, fmaf(w1, t[1].y, w0 * t[0].y)));
  v.z = fmaf(w3, t[3].z, fmaf(w2, t[2].z, fmaf(w1, t[1].z, w0 * t[0].z)));
  v.w = fmaf(w3, t[3].w, fmaf(w2, t[2].w, fmaf(w1, t[1].w, w0 * t[0].w)));
  return v;
}
// the same for one channel
LP_DEV float kp_fold1(const float* t, float w0, float w1, float w2, float w3) {
  return fmaf(w3, t[3], fmaf(w2, t[2], fmaf(w1, t[1], w0 * t[0])));
}

// the 4 vertices of the P planes of scale s at this lane's float4 of channels (float offset c0), all loads issued together
template <int P>
LP_DEV void kp_load_taps(const LpKPlanesArgs& a, const KpCell& c, int b, int s, int c0, float4 (*tap)[4]) {
  const int64_t C = a.channels;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const float* v0 = a.planes + kp_base_row(a, c, b, s, j) * C + c0;
    const float* v1 = v0 + (int64_t)c.n * C;
    tap[j][0] = kp_ld4(v0);
    tap[j][1] = kp_ld4(v0 + C);
    tap[j][2] = kp_ld4(v1);
    tap[j][3] = kp_ld4(v1 + C);
  }
}

// the four vertex sums of one plane go to the rows base, base + 1, base + n, base + n + 1 of the gradient tensor: a group of C lanes
// writes a whole row per instruction
LP_DEV void kp_flush(float* grad, int64_t base, int n, int64_t C, int c, float* sum) {
  float* v0 = grad + base * C + c;
  float* v1 = v0 + (int64_t)n * C;
  atomic_add_f32(v0, sum[0]);
  atomic_add_f32(v0 + C, sum[1]);
  atomic_add_f32(v1, sum[2]);
  atomic_add_f32(v1 + C, sum[3]);
  sum[0] = sum[1] = sum[2] = sum[3] = 0.0f;
}

// a point's geometry on one scale, as lane = point leaves it in an LDS tile for lanes = channels: KP_LD(P) words per point -- per
// plane (row low word, row high word, f_u, f_v), then the bits of the spatial axes that were not clamped; odd: no bank conflicts.
// A masked point or a lane past the end (`on` false) leaves a negative row.
#define KP_LD(P) (4 * (P) + 1)

template <int P>
LP_DEV void kp_tile_store(const LpKPlanesArgs& a, const KpCell& c, int b, int s, bool on, float* e) {
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int64_t row = on ? kp_base_row(a, c, b, s, j) : (int64_t)-1;
    e[4 * j + 0] = __int_as_float((int)(row & 0xffffffff));
    e[4 * j + 1] = __int_as_float((int)(row >> 32));
    e[4 * j + 2] = c.ax[KP_U(j)].f;
    e[4 * j + 3] = c.ax[KP_V(j)].f;
  }
  e[4 * P] = __int_as_float((c.ax[0].free ? 1 : 0) | (c.ax[1].free ? 2 : 0) | (c.ax[2].free ? 4 : 0));
}

LP_DEV int64_t kp_tile_row(const float* e, int j) {
  return ((int64_t)__float_as_int(e[4 * j + 1]) << 32) | (int64_t)(unsigned)__float_as_int(e[4 * j]);
}

}  // namespace lp

// lp_plane_range.h -- which samples of a PLAIN march (depth_s = near + lin01(s, S) (far - near), no contraction, no beyond-far tail)
// can reach a grid at all.  One definition for the kernels (lp_mfma_common.h: wave_plane_ranges) and for the host program that
// checks it by brute force (tests/host/plane_range_check.cpp); no HIP dependency, so a plain C++ compiler can build it.
//
// A bilinear tap of a grid axis with `size` cells carries weight only while the un-normalised coordinate
// t = ((c + 1) size - 1) / 2 lies in (-1, size): the slab |c| < 1 + 1 / size (the cube widened by the border that axis_taps /
// axis_norm interpolate against zero).  c = depth * d + o is linear in the depth, so the depths inside the slab are ONE interval; a
// plane needs two slabs at once, a voxel grid three: intersections of intervals.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define LP_HD __host__ __device__ inline
#else
#define LP_HD inline
#endif

namespace lp {

struct SampleSpan {
  int lo, hi;  // samples lo .. hi (inclusive) may carry weight; lo > hi: none does
};

LP_HD SampleSpan span_full(int S) { return SampleSpan{0, S - 1}; }
LP_HD SampleSpan span_none(int S) { return SampleSpan{S, -1}; }
LP_HD SampleSpan span_meet(SampleSpan a, SampleSpan b, int S) {  // both
  const SampleSpan m{a.lo > b.lo ? a.lo : b.lo, a.hi < b.hi ? a.hi : b.hi};
  return m.lo > m.hi ? span_none(S) : m;
}
LP_HD SampleSpan span_hull(SampleSpan a, SampleSpan b) {  // either (span_none is its neutral element)
  return SampleSpan{a.lo < b.lo ? a.lo : b.lo, a.hi > b.hi ? a.hi : b.hi};
}

// Samples at which the coordinate depth * d + o of one axis is inside the slab of a grid axis with `size` cells.
// The slab's two depths are turned into (fractional) sample indices and rounded OUTWARD by one whole sample; `err` bounds, in
// samples, what the float arithmetic here and in the march (depth, point, un-normalisation: a few ulp of the terms involved) can
// move a crossing.  Where it is not safely below that one sample -- a ray (nearly) parallel to the slab, near == far, non-finite
// input (the comparison is false for NaN) -- the answer is "every sample".
LP_HD SampleSpan axis_sample_span(float o, float d, float near_t, float far_t, int S, int size) {
  if (S < 2) return span_full(S);
  const float L = 1.0f + 1.0f / (float)size;
  const float per = (float)(S - 1) / (far_t - near_t);  // samples per unit of depth (signed)
  const float inv = 1.0f / d;
  float s0 = ((-L - o) * inv - near_t) * per;
  float s1 = ((L - o) * inv - near_t) * per;
  if (s0 > s1) { const float t = s0; s0 = s1; s1 = t; }
  const float err = 1.9073486e-6f * fabsf(per) * ((L + fabsf(o)) * fabsf(inv) + fabsf(near_t) + fabsf(far_t));  // 16 * 2^-23
  if (!(err < 0.5f)) return span_full(S);
  if (!(s0 <= (float)S && s1 >= -1.0f)) return span_none(S);  // the slab lies behind the last / before the first sample
  const int lo = (int)floorf(fmaxf(s0, 0.0f)) - 1;
  const int hi = (int)ceilf(fminf(s1, (float)(S - 1))) + 1;
  return SampleSpan{lo < 0 ? 0 : lo, hi > S - 1 ? S - 1 : hi};
}

// The three slabs of one ray: x against W cells, y against H, z against D.
struct AxisSpans {
  SampleSpan x, y, z;
};
LP_HD AxisSpans ray_axis_spans(float ox, float oy, float oz, float dx, float dy, float dz, float near_t, float far_t, int S, int W,
                               int H, int D) {
  return AxisSpans{axis_sample_span(ox, dx, near_t, far_t, S, W), axis_sample_span(oy, dy, near_t, far_t, S, H),
                   axis_sample_span(oz, dz, near_t, far_t, S, D)};
}
// plane g of a canonical triplane: 0 = xy, 1 = xz, 2 = yz
LP_HD SampleSpan plane_span(const AxisSpans& a, int g, int S) {
  return g == 0 ? span_meet(a.x, a.y, S) : (g == 1 ? span_meet(a.x, a.z, S) : span_meet(a.y, a.z, S));
}
LP_HD SampleSpan voxel_span(const AxisSpans& a, int S) { return span_meet(span_meet(a.x, a.y, S), a.z, S); }

}  // namespace lp

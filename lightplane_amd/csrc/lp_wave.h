// lp_wave.h -- sums and scans over the 64 lanes of a wavefront, shared by the one-wavefront-per-ray kernels (lp_composite.hip,
// lp_importance.hip) and the mesh's counting passes (lp_mesh.hip).  The float scans add the shifted copy under a lane mask (an
// exclusive value is the inclusive one shifted by a lane, never `inclusive - x`: no cancellation).
#pragma once

#include "lp_device.h"

namespace lp {

LP_DEV float wave_sum(float x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
  return x;
}
// inclusive prefix sum over the wave, lane 0 first
template <typename T>
LP_DEV T wave_scan(T x, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  return x;
}
// inclusive suffix sum over the wave, lane 63 first
LP_DEV float wave_rscan(float x, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float y = __shfl_down(x, d, 64);
    if (lane + d < 64) x += y;
  }
  return x;
}


// The two helpers of the kernels that render one ray per wave at caller-given depths (lp_render_samples.hip, lp_hash_render.hip).
// The ray of a sample_point() call: origin and direction of row r, batch element b, no near / far.
LP_DEV Ray sample_ray(const float* origins, const float* directions, int64_t r, int b) {
  Ray q;
  load_ray_line(origins, directions, r, q);
  q.near_t = q.far_t = 0.0f;
  q.b = b;
  return q;
}

// sum + p[0] + p[stride] + ... + p[63 * stride] in that order (LDS), the reads issued sixteen at a time: one dependent read per add
// is 64 LDS latencies per call
LP_DEV float column_sum(const float* p, int stride, float sum) {
  for (int j0 = 0; j0 < 64; j0 += 16) {
    float v[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] = p[(j0 + q) * stride];
#pragma unroll
    for (int q = 0; q < 16; ++q) sum += v[q];
  }
  return sum;
}

}  // namespace lp

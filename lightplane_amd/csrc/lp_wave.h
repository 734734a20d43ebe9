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

}  // namespace lp

// lp_rows.h -- access to the channel rows of a channels-last tensor, shared by the stand-alone ops: one unit of V floats per access
// (V = 4: 16 bytes where the channel count and the pointers allow it, V = 1 otherwise), the host rule that picks V, and the in-place
// division of rows by their clamped weight (lp_splatter.hip, lp_point_grid.hip).
#pragma once

#include <initializer_list>

#include "lp_device.h"

namespace lp {

template <int V>
struct Vec {
  float v[V];
};

template <int V>
LP_DEV Vec<V> vec_load(const float* p) {
  Vec<V> r;
  if constexpr (V == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    r.v[0] = t.x, r.v[1] = t.y, r.v[2] = t.z, r.v[3] = t.w;
  } else {
    r.v[0] = *p;
  }
  return r;
}

template <int V>
LP_DEV void vec_store(float* p, const Vec<V>& r) {
  if constexpr (V == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
  } else {
    *p = r.v[0];
  }
}

// host: floats per access for rows of `channels` floats behind these base pointers -- 4 where C % 4 == 0 and every pointer is 16-byte
// aligned (a row then starts on a 16-byte boundary: row * C * 4 bytes behind an aligned base), else 1
inline int row_vec(int channels, std::initializer_list<const void*> ptrs) {
  if ((channels & 3) != 0) return 1;
  for (const void* p : ptrs)
    if (((uintptr_t)p & 15) != 0) return 1;
  return 4;
}

// feature[row][:] /= max(weight[row], 1e-5) in place, grid-stride over blockIdx.x of a 256-thread launch.  True division (matches
// torch's feat / clamp(weight)): the pass is HBM bound anyway.  C % 4 == 0: 16 bytes per access, `feature` 16-byte aligned.
LP_DEV void normalize_rows(float* feature, const float* weight, int64_t n_rows, int C) {
  const int64_t n = n_rows * C;
  const int64_t stride = (int64_t)gridDim.x * 256;
  if ((C & 3) == 0) {
    const int64_t n4 = n / 4;
    const int c4 = C / 4;
    float4* f4 = reinterpret_cast<float4*>(feature);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
      float4 v = f4[i];
      const float d = fmaxf(weight[i / c4], 1e-5f);
      v.x = v.x / d; v.y = v.y / d; v.z = v.z / d; v.w = v.w / d;
      f4[i] = v;
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) feature[i] = feature[i] / fmaxf(weight[i / C], 1e-5f);
  }
}

}  // namespace lp

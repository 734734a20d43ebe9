// lp_launch.h -- how many workgroups a launch needs.  One definition for every launcher (launch_blocks, lp_host.h) and for the host
// program that checks it (tests/host/launch_blocks_check.cpp); no HIP dependency, so a plain C++ compiler can build it.
#pragma once
#include <stdint.h>

namespace lp {

// a grid dimension is handed to the runtime as a 32-bit value, and the kernels form blockIdx.x * (items per workgroup) from it
constexpr int64_t LP_MAX_WORKGROUPS = ((int64_t)1 << 31) - 1;

// Workgroups of `per` items (> 0) that cover `items` (>= 0): ceil(items / per), formed without the overflow `items + per - 1` has near
// INT64_MAX; 0 items need 0 workgroups.  False where the count cannot be launched; `count` is set either way (for the message).
inline bool workgroup_count(int64_t items, int64_t per, int64_t& count) {
  count = items / per + (items % per != 0 ? 1 : 0);
  return count <= LP_MAX_WORKGROUPS;
}

}  // namespace lp

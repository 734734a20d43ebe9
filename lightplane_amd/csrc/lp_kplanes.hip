// lp_kplanes.hip -- space-time plane encoding of 3-D points with a timestamp (K-Planes / HexPlane; without time planes the Hadamard
// tri-plane), forward and both gradients (C ABI lp_kplanes_forward / lp_kplanes_backward_planes /
// lp_kplanes_backward_points, include/lightplane_hip_kplanes.h, which holds the definition).  The layout (vertices per axis and first
// row of every plane of every scale) is the caller's: the kernels read it from the argument block with a wave-uniform index.
//   kplanes_fwd<P>                 work item (point, scale, float4 of channels): C / 4 consecutive lanes serve one point, blockIdx.y =
//                                  SCALE, the slow index of the launch -- the workgroups in flight at one time read one scale's planes.
//                                  Every lane forms the point's geometry itself (4.14: per-lane geometry beat an LDS-shared form),
//                                  issues the 4 P vertex loads of 16 bytes before the first use, folds them into the P plane values,
//                                  multiplies those and stores one float4: the [point][S C] store is contiguous over the lanes of a
//                                  point.  No LDS, no atomics.
//   kplanes_bwd_planes<P, CW_LOG>  one wave per 64 consecutive points of one scale.  Phase 1, lane = point: geometry; per plane the base
//                                  row (64 bit) and the two fractions go to an LDS tile, a masked point or a lane past the end leaves a
//                                  negative row.  Phase 2, lanes = channels: a group of CW = C lanes walks CW consecutive points of the
//                                  tile (64 / CW groups side by side), recomputes the P values from their 4 vertices, forms the product
//                                  of the OTHER values by a prefix / suffix pass (no division: values may be 0) times the upstream
//                                  gradient, and keeps four vertex sums per plane in registers.  RUN MERGING: the sums of a plane are
//                                  added to memory (one atomic instruction per vertex, whole rows of 4 C contiguous bytes) only when
//                                  the next point's base row on that plane differs, or after the group's last point.  Consecutive
//                                  samples of a ray share cells on the coarse scales, and with one timestamp per ray the time index is
//                                  constant: the merge is per plane, not per point.
//   kplanes_bwd_points<P>          C / 4 lanes per point, loop over the scales: per axis the channel slice of sum_j (d v_j / d axis)
//                                  prod_{i != j} v_i g, scaled by (n_s - 1) / 2 (0 on a clamped axis), reduced over the lanes of the
//                                  point with xor shuffles (commutative adds: every lane holds the same bits), contract_backward, one
//                                  lane stores the three floats.  Fixed order, no atomics.
// 64-bit row offsets throughout; no workspace; nothing but the caller's buffers is written.
#include "lp_kplanes_planes.h"

namespace lp {

// (the axis map, point, cell, base row, KP_U / KP_V, folds and flush: lp_kplanes_planes.h)

struct KpArgs {
  LpKPlanesArgs a;
  int64_t n_points;
  int32_t lanes_log;  // log2(C / 4): lanes per point of the forward and the point gradient
};

template <int P>
__global__ void __launch_bounds__(256) kplanes_fwd(const KpArgs s) {
  const LpKPlanesArgs& a = s.a;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t p = gid >> s.lanes_log;
  if (p >= s.n_points) return;
  const int c0 = 4 * (int)(gid & ((1 << s.lanes_log) - 1));
  const int sc = blockIdx.y;
  const KpPoint pt = kp_point<P>(a, p);
  float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (pt.inside) {
    const KpCell c = kp_cell<P>(a, pt, sc);
    float4 tap[P][4];
    kp_load_taps<P>(a, c, pt.ray.b, sc, c0, tap);
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const float fu = c.ax[KP_U(j)].f, fv = c.ax[KP_V(j)].f;
      const float gu = 1.0f - fu, gv = 1.0f - fv;
      const float4 v = kp_fold(tap[j], gu * gv, fu * gv, gu * fv, fu * fv);
      acc = j == 0 ? v : kp_mul(acc, v);
    }
  }
  *reinterpret_cast<float4*>(a.out_features + p * ((int64_t)a.n_scales * a.channels) + sc * a.channels + c0) = acc;
}

template <int P>
__global__ void __launch_bounds__(256) kplanes_bwd_points(const KpArgs s) {
  const LpKPlanesArgs& a = s.a;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t pg = gid >> s.lanes_log;
  const bool live = pg < s.n_points;  // (the lanes of a point are live together; a dead group looks at point 0 and stores nothing)
  const int64_t p = live ? pg : 0;
  const int lane_c = (int)(gid & ((1 << s.lanes_log) - 1));
  const int c0 = 4 * lane_c;
  const KpPoint pt = kp_point<P>(a, p);
  float g3[3] = {0.0f, 0.0f, 0.0f};
  if (pt.inside) {
    const int64_t SC = (int64_t)a.n_scales * a.channels;
    for (int sc = 0; sc < a.n_scales; ++sc) {
      const KpCell c = kp_cell<P>(a, pt, sc);
      float4 tap[P][4];
      kp_load_taps<P>(a, c, pt.ray.b, sc, c0, tap);
      const float4 g = kp_ld4(a.grad_features + p * SC + sc * a.channels + c0);
      float4 v[P], du[P], dv[P];
#pragma unroll
      for (int j = 0; j < P; ++j) {
        const float fu = c.ax[KP_U(j)].f, fv = c.ax[KP_V(j)].f;
        const float gu = 1.0f - fu, gv = 1.0f - fv;
        v[j] = kp_fold(tap[j], gu * gv, fu * gv, gu * fv, fu * fv);
        du[j] = kp_fold(tap[j], -gv, gv, -fv, fv);  // d v_j / d f_u
        dv[j] = kp_fold(tap[j], -gu, -fu, gu, fu);  // d v_j / d f_v
      }
      // o_j = g * prod_{i != j} v_i: prefix products going up, suffix products coming down
      float4 o[P];
      float4 run = g;
#pragma unroll
      for (int j = 0; j < P; ++j) {
        o[j] = run;
        run = kp_mul(run, v[j]);
      }
      run = v[P - 1];
#pragma unroll
      for (int j = P - 2; j >= 0; --j) {
        o[j] = kp_mul(o[j], run);
        run = kp_mul(run, v[j]);
      }
      float acc[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int j = 0; j < P; ++j) {
        acc[KP_U(j)] += kp_dot(du[j], o[j]);
        if (KP_V(j) < 3) acc[KP_V(j)] += kp_dot(dv[j], o[j]);
      }
      const float half = 0.5f * (float)(c.n - 1);
#pragma unroll
      for (int x = 0; x < 3; ++x) g3[x] = fmaf(c.ax[x].free ? half : 0.0f, acc[x], g3[x]);
    }
  }
  for (int d = 1; d < (1 << s.lanes_log); d <<= 1) {
#pragma unroll
    for (int x = 0; x < 3; ++x) g3[x] += __shfl_xor(g3[x], d, 64);
  }
  if (pt.inside && a.contract_coords) contract_backward(pt.ray.ox, pt.ray.oy, pt.ray.oz, g3[0], g3[1], g3[2]);
  if (live && lane_c == 0) {
    float* gp = a.grad_points + 3 * p;
    gp[0] = g3[0];
    gp[1] = g3[1];
    gp[2] = g3[2];
  }
}

template <int P, int CW_LOG>
__global__ void __launch_bounds__(64) kplanes_bwd_planes(const KpArgs s) {
  constexpr int LD = 4 * P + 1;   // words per point of the tile: per plane (row low word, row high word, f_u, f_v); odd, no bank conflicts
  constexpr int CW = 1 << CW_LOG;  // lanes per row = C = points a group walks
  __shared__ float tile[64 * LD];
  const LpKPlanesArgs& a = s.a;
  const int lane = threadIdx.x;
  const int sc = blockIdx.y;
  const int64_t first = (int64_t)blockIdx.x * 64;
  {
    // phase 1: lane = point
    const bool live = first + lane < s.n_points;
    const KpPoint pt = kp_point<P>(a, live ? first + lane : 0);  // (a lane past the end looks at point 0 and contributes nothing)
    const bool on = live && pt.inside;
    const KpCell c = kp_cell<P>(a, pt, sc);
    float* e = tile + lane * LD;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const int64_t row = on ? kp_base_row(a, c, pt.ray.b, sc, j) : (int64_t)-1;
      e[4 * j + 0] = __int_as_float((int)(row & 0xffffffff));
      e[4 * j + 1] = __int_as_float((int)(row >> 32));
      e[4 * j + 2] = c.ax[KP_U(j)].f;
      e[4 * j + 3] = c.ax[KP_V(j)].f;
    }
  }
  __syncthreads();
  // phase 2: lanes = channels; group `sub` walks the points sub * CW .. sub * CW + CW - 1 of the tile
  const int sub = lane >> CW_LOG, c = lane & (CW - 1);
  const int n = a.spatial[sc];
  const int64_t C = CW;
  const int64_t SC = (int64_t)a.n_scales * C;
  float sum[P][4];
  int64_t held[P];  // base row the sums of plane j belong to; negative: none
#pragma unroll
  for (int j = 0; j < P; ++j) {
    held[j] = -1;
    sum[j][0] = sum[j][1] = sum[j][2] = sum[j][3] = 0.0f;
  }
  for (int t = 0; t < CW; ++t) {
    const int r = sub * CW + t;  // < 64
    const float* e = tile + r * LD;
    int64_t row[P];
    float fu[P], fv[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
      row[j] = ((int64_t)__float_as_int(e[4 * j + 1]) << 32) | (int64_t)(unsigned)__float_as_int(e[4 * j]);
      fu[j] = e[4 * j + 2];
      fv[j] = e[4 * j + 3];
    }
    if (row[0] < 0) continue;  // masked or past the end (uniform over the group): the held runs go on
    float tap[P][4];
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const float* v0 = a.planes + row[j] * C + c;
      const float* v1 = v0 + (int64_t)n * C;
      tap[j][0] = v0[0];
      tap[j][1] = v0[C];
      tap[j][2] = v1[0];
      tap[j][3] = v1[C];
    }
    const float g = a.grad_features[(first + r) * SC + sc * CW + c];
    float w[P][4], v[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const float gu = 1.0f - fu[j], gv = 1.0f - fv[j];
      w[j][0] = gu * gv; w[j][1] = fu[j] * gv; w[j][2] = gu * fv[j]; w[j][3] = fu[j] * fv[j];
      v[j] = fmaf(w[j][3], tap[j][3], fmaf(w[j][2], tap[j][2], fmaf(w[j][1], tap[j][1], w[j][0] * tap[j][0])));
    }
    // o_j = g * prod_{i != j} v_i
    float o[P];
    float run = g;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      o[j] = run;
      run *= v[j];
    }
    run = v[P - 1];
#pragma unroll
    for (int j = P - 2; j >= 0; --j) {
      o[j] *= run;
      run *= v[j];
    }
#pragma unroll
    for (int j = 0; j < P; ++j) {
      if (held[j] != row[j]) {  // (uniform over the group) the run of plane j ends here
        if (held[j] >= 0) kp_flush(a.grad_planes, held[j], n, C, c, sum[j]);
        held[j] = row[j];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) sum[j][k] = fmaf(w[j][k], o[j], sum[j][k]);
    }
  }
#pragma unroll
  for (int j = 0; j < P; ++j)
    if (held[j] >= 0) kp_flush(a.grad_planes, held[j], n, C, c, sum[j]);
}

// ---------------------------------------------------------------------------------------------------------------------------
// host side (`a` checked by lp_api.hip; n_rays * n_pts > 0)
// ---------------------------------------------------------------------------------------------------------------------------

static int log2_of(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

#define LP_KP_LAUNCH(kernel, grid)                                              \
  if (a.n_planes == 3)                                                          \
    hipLaunchKernelGGL(kernel<3>, grid, dim3(256), 0, stream, s);               \
  else                                                                          \
    hipLaunchKernelGGL(kernel<6>, grid, dim3(256), 0, stream, s);

#define LP_KP_PLANES(P)                                                                                           \
  switch (a.channels) {                                                                                           \
    case 4: hipLaunchKernelGGL((kplanes_bwd_planes<P, 2>), grid, dim3(64), 0, stream, s); break;                  \
    case 8: hipLaunchKernelGGL((kplanes_bwd_planes<P, 3>), grid, dim3(64), 0, stream, s); break;                  \
    case 16: hipLaunchKernelGGL((kplanes_bwd_planes<P, 4>), grid, dim3(64), 0, stream, s); break;                 \
    case 32: hipLaunchKernelGGL((kplanes_bwd_planes<P, 5>), grid, dim3(64), 0, stream, s); break;                 \
    default: hipLaunchKernelGGL((kplanes_bwd_planes<P, 6>), grid, dim3(64), 0, stream, s); break;                 \
  }

// mode: 0 forward, 1 backward_planes, 2 backward_points
static int kplanes_launch(const char* what, const LpKPlanesArgs& a, int mode, hipStream_t stream) {
  KpArgs s;
  s.a = a;
  s.n_points = a.n_rays * a.n_pts;
  s.lanes_log = log2_of(a.channels / 4);
  unsigned blocks;
  if (mode == 1) {
    if (int rc = launch_blocks(what, s.n_points, 64, blocks)) return rc;
    const dim3 grid(blocks, (unsigned)a.n_scales);  // x runs fastest: a scale's workgroups are dispatched together
    if (a.n_planes == 3) {
      LP_KP_PLANES(3)
    } else {
      LP_KP_PLANES(6)
    }
  } else {
    if (int rc = launch_blocks(what, s.n_points << s.lanes_log, 256, blocks)) return rc;
    if (mode == 0) {
      LP_KP_LAUNCH(kplanes_fwd, dim3(blocks, (unsigned)a.n_scales))
    } else {
      LP_KP_LAUNCH(kplanes_bwd_points, dim3(blocks))
    }
  }
  return check_launch(what);
}

int kplanes_forward_launch(const LpKPlanesArgs& a, hipStream_t stream) { return kplanes_launch("lp_kplanes_forward", a, 0, stream); }
int kplanes_backward_planes_launch(const LpKPlanesArgs& a, hipStream_t stream) {
  return kplanes_launch("lp_kplanes_backward_planes", a, 1, stream);
}
int kplanes_backward_points_launch(const LpKPlanesArgs& a, hipStream_t stream) {
  return kplanes_launch("lp_kplanes_backward_points", a, 2, stream);
}

const char* build_info_kplanes() {
  return "{\"forward\": \"C / 4 lanes per (point, scale), one float4 of channels per lane, scale = slow launch index; geometry per lane, "
         "4 P vertex loads in flight, product of the P bilinear values; no LDS, no atomics\", \"backward_planes\": \"one wave per 64 "
         "points of a scale; base rows and fractions through LDS, lanes = channels: groups of C lanes walk consecutive points, product "
         "of the other planes by a prefix / suffix pass (no division), four vertex sums per plane in registers, whole-row fp32 atomics "
         "only where a plane's base row changes (run merging per plane)\", \"backward_points\": \"C / 4 lanes per point, loop over the "
         "scales, xor-shuffle sum over the point's lanes, stored\"}";
}

}  // namespace lp

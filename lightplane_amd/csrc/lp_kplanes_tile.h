// lp_kplanes_tile.h -- the two lanes = channels passes over a 64-point geometry tile geo[64][KP_LD(P)] (kp_tile_store,
// lp_kplanes_planes.h) that the fused plane-field kernels share: the decoder at points (lp_kplanes_points.hip) and the render along
// rays (lp_kplanes_render.hip).  kpp_gather loads whole plane rows and leaves the features of a scale in an LDS tile; kpp_walk is the
// run-merged scatter of d feat into grad_planes (and, at points, the point gradient).  The arithmetic and its order are the same in
// every caller: the same bits.
#pragma once
#include "lp_kplanes_planes.h"

namespace lp {

// lanes = channels, float4 slices: the features of scale s of the tile's 64 points from geo[64][KP_LD(P)] into
// dst[point * pstride + (s C + c) * cstride]; a negative row gives zeros.  Every lane of the wave calls this.
template <int P>
LP_DEV void kpp_gather(const LpKPlanesArgs& g, const float* geo, int s, int lanes_log, int lane, float* dst, int pstride, int cstride) {
  const int per = 64 >> lanes_log;  // points per pass
  const int c0 = 4 * (lane & ((1 << lanes_log) - 1));
  const int n = g.spatial[s];
  const int64_t C = g.channels;
  for (int pass = 0; pass < (1 << lanes_log); ++pass) {
    const int r = pass * per + (lane >> lanes_log);  // < 64
    const float* e = geo + r * KP_LD(P);
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (kp_tile_row(e, 0) >= 0) {
      float4 tap[P][4];
#pragma unroll
      for (int j = 0; j < P; ++j) {
        const float* v0 = g.planes + kp_tile_row(e, j) * C + c0;
        const float* v1 = v0 + (int64_t)n * C;
        tap[j][0] = kp_ld4(v0);
        tap[j][1] = kp_ld4(v0 + C);
        tap[j][2] = kp_ld4(v1);
        tap[j][3] = kp_ld4(v1 + C);
      }
#pragma unroll
      for (int j = 0; j < P; ++j) {
        const float fu = e[4 * j + 2], fv = e[4 * j + 3];
        const float gu = 1.0f - fu, gv = 1.0f - fv;
        const float4 v = kp_fold(tap[j], gu * gv, fu * gv, gu * fv, fu * fv);
        acc = j == 0 ? v : kp_mul(acc, v);
      }
    }
    float* d = dst + r * pstride + (s * (int)C + c0) * cstride;
    d[0] = acc.x;
    d[cstride] = acc.y;
    d[2 * cstride] = acc.z;
    d[3 * cstride] = acc.w;
  }
}

// lanes = channels, one channel per lane: scale s of the tile.  Group `sub` of CW = C lanes walks the points sub * CW .. of geo; dfeat:
// the staged d feat [64][ld]; pg: [64][3] point-gradient sums (used when g.grad_points).  Every lane of the wave calls this; all
// groups make the same number of steps, so the shuffles meet every lane.
template <int P>
LP_DEV void kpp_walk(const LpKPlanesArgs& g, const float* geo, const float* dfeat, int ld, int s, int cw_log, int lane, float* pg) {
  const int CW = 1 << cw_log;
  const int sub = lane >> cw_log, c = lane & (CW - 1);
  const int n = g.spatial[s];
  const int64_t C = CW;
  const bool want_planes = g.grad_planes != nullptr, want_points = g.grad_points != nullptr;  // wave-uniform
  const float half = 0.5f * (float)(n - 1);
  float sum[P][4];
  int64_t held[P];  // base row the sums of plane j belong to; negative: none
#pragma unroll
  for (int j = 0; j < P; ++j) {
    held[j] = -1;
    sum[j][0] = sum[j][1] = sum[j][2] = sum[j][3] = 0.0f;
  }
  for (int t = 0; t < CW; ++t) {
    const int r = sub * CW + t;  // < 64
    const float* e = geo + r * KP_LD(P);
    const bool on = kp_tile_row(e, 0) >= 0;  // (uniform over the group) not masked, not past the end
    float acc[3] = {0.0f, 0.0f, 0.0f};
    if (on) {
      int64_t row[P];
      float fu[P], fv[P];
      float tap[P][4];
#pragma unroll
      for (int j = 0; j < P; ++j) {
        row[j] = kp_tile_row(e, j);
        fu[j] = e[4 * j + 2];
        fv[j] = e[4 * j + 3];
        const float* v0 = g.planes + row[j] * C + c;
        const float* v1 = v0 + (int64_t)n * C;
        tap[j][0] = v0[0];
        tap[j][1] = v0[C];
        tap[j][2] = v1[0];
        tap[j][3] = v1[C];
      }
      const float gf = dfeat[r * ld + s * CW + c];
      float w[P][4], v[P];
#pragma unroll
      for (int j = 0; j < P; ++j) {
        const float gu = 1.0f - fu[j], gv = 1.0f - fv[j];
        w[j][0] = gu * gv; w[j][1] = fu[j] * gv; w[j][2] = gu * fv[j]; w[j][3] = fu[j] * fv[j];
        v[j] = kp_fold1(tap[j], w[j][0], w[j][1], w[j][2], w[j][3]);
      }
      // o_j = g * prod_{i != j} v_i: prefix products going up, suffix products coming down
      float o[P];
      float run = gf;
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
      if (want_planes) {
#pragma unroll
        for (int j = 0; j < P; ++j) {
          if (held[j] != row[j]) {  // (uniform over the group) the run of plane j ends here
            if (held[j] >= 0) kp_flush(g.grad_planes, held[j], n, C, c, sum[j]);
            held[j] = row[j];
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) sum[j][k] = fmaf(w[j][k], o[j], sum[j][k]);
        }
      }
      if (want_points) {
#pragma unroll
        for (int j = 0; j < P; ++j) {
          const float gu = 1.0f - fu[j], gv = 1.0f - fv[j];
          const float du = kp_fold1(tap[j], -gv, gv, -fv[j], fv[j]);  // d v_j / d f_u
          acc[KP_U(j)] = fmaf(du, o[j], acc[KP_U(j)]);
          if (KP_V(j) < 3) {
            const float dv = kp_fold1(tap[j], -gu, -fu[j], gu, fu[j]);  // d v_j / d f_v
            acc[KP_V(j)] = fmaf(dv, o[j], acc[KP_V(j)]);
          }
        }
      }
    }
    if (want_points) {
      for (int d = 1; d < CW; d <<= 1) {
#pragma unroll
        for (int x = 0; x < 3; ++x) acc[x] += __shfl_xor(acc[x], d, 64);
      }
      if (on && c == 0) {
        const int free_bits = __float_as_int(e[4 * P]);
#pragma unroll
        for (int x = 0; x < 3; ++x) pg[3 * r + x] = fmaf(((free_bits >> x) & 1) ? half : 0.0f, acc[x], pg[3 * r + x]);
      }
    }
  }
  if (want_planes) {
#pragma unroll
    for (int j = 0; j < P; ++j)
      if (held[j] >= 0) kp_flush(g.grad_planes, held[j], n, C, c, sum[j]);
  }
}

}  // namespace lp

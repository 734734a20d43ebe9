// lp_grid_resample.hip -- resample the grids of a grid-list to new spatial sizes (tri- / bi-linear), forward and adjoint, directly on
// the channels-last layout [B, D, H, W, C]: no permute, no temporaries.
//
// Per spatial axis with input extent n_in, output extent n_out and ONE fp32 host coefficient a:
//   align_corners: src(o) = a * o;   otherwise: src(o) = max(0, a * (o + 0.5) - 0.5)      (every operation individually rounded)
//   i0 = min(floor(src), n_in - 1), i1 = min(i0 + 1, n_in - 1), lambda = clamp(src - i0, 0, 1)
// out[o] = sum over the 8 corners of prod_axis (1 - lambda | lambda) * in[corner]; batch and channel axes are never resampled.  This is
// torch.nn.functional.interpolate (trilinear; bilinear for a plane, whose singular axis has i0 = i1 = 0 and weights that sum to 1).
//
// rs_tap() below is the ONE place that evaluates (i0, i1, lambda); forward and adjoint both call it, so the adjoint's weights are the
// forward's by construction.
//
// Forward, output-stationary: a lane owns one (output cell, channel group); the 256 lanes of a workgroup are 256 consecutive groups
// of an output slice (4 KB, one contiguous store per wave instruction).  Workgroups are numbered tile-fastest, then z, then batch, so
// the resident ones cover consecutive tiles of the same output slice(s): their inputs are two (at a slice change three) input
// slices, and the 8-fold reuse of every input row is served by L1 / L2.  No LDS.
// Adjoint, input-stationary gather (no atomics: bit-reproducible): a lane owns one (input cell, channel group).  Per axis it takes the
// candidate outputs from the inverse mapping, widened by a margin, narrows the range to the outputs whose recomputed taps touch its
// cell (they are contiguous: src is monotone in o), and sums weight * grad_out over the box in a fixed order (z, y, x ascending).
// Correct for any size ratio (an input cell no output touches gets 0); the margin only costs time.
#include "lp_host.h"
#include "lp_rows.h"

namespace lp {

constexpr int RS_THREADS = 256;

struct RsGrid {
  const float* in;   // forward: the source grid; adjoint: the gradient w.r.t. the destination (what the lane GATHERS from)
  float* out;        // forward: the destination; adjoint: the gradient w.r.t. the source (what the lane owns)
  int32_t B;
  int32_t sn[3];     // source extents  D, H, W
  int32_t dn[3];     // destination extents D, H, W
  float a[3];        // coordinate coefficients D, H, W
  float ia[3];       // adjoint: 1 / a (0 where a == 0: every output is a candidate)
  int32_t align;
  int32_t cgn;       // lane positions per cell: C / VEC
  uint32_t tiles;    // ceil(H * W * cgn / RS_THREADS) of the lane-owning side
};

struct RsTap {
  int32_t i0, i1;
  float w0, w1;  // 1 - lambda, lambda
};

// the definition: the two input cells output cell `o` of an axis reads and their weights
LP_DEV RsTap rs_tap(int32_t o, float a, int32_t align, int32_t n_in) {
  float src;
  if (align) {
    src = a * (float)o;
  } else {
    src = a * ((float)o + 0.5f);
    src = src - 0.5f;
    src = fmaxf(src, 0.0f);
  }
  RsTap t;
  // (src is finite and >= 0; the comparison in float keeps the conversion in range for any coefficient)
  t.i0 = src >= (float)(n_in - 1) ? n_in - 1 : (int32_t)floorf(src);
  t.i1 = min(t.i0 + 1, n_in - 1);
  const float l = fminf(fmaxf(src - (float)t.i0, 0.0f), 1.0f);
  t.w0 = 1.0f - l;
  t.w1 = l;
  return t;
}

// (b, z, y, x, first float of the channel group) of the lane; false past the end of the slice
struct RsLane {
  int32_t b, z, y, x;
  int32_t c0;
};

template <int VEC>
LP_DEV bool rs_lane(const RsGrid& a, const int32_t* n, RsLane& l) {
  const uint32_t bid = blockIdx.x;
  const uint32_t tile = bid % a.tiles;
  const uint32_t rest = bid / a.tiles;
  l.z = (int32_t)(rest % (uint32_t)n[0]);
  l.b = (int32_t)(rest / (uint32_t)n[0]);
  const int64_t items = (int64_t)n[1] * n[2] * a.cgn;  // lane positions per slice
  const int64_t j = (int64_t)tile * RS_THREADS + threadIdx.x;
  if (j >= items) return false;
  const int64_t cell = j / a.cgn;  // y * W + x
  l.c0 = (int32_t)(j - cell * a.cgn) * VEC;
  l.x = (int32_t)(cell % n[2]);
  l.y = (int32_t)(cell / n[2]);
  return true;
}

// row of cell (b, z, y, x) in a grid of extents n: below 2^31 (checked on the host); element offsets are 64-bit
LP_DEV int64_t rs_elem(const int32_t* n, int32_t b, int32_t z, int32_t y, int32_t x, int32_t channels) {
  const int32_t row = ((b * n[0] + z) * n[1] + y) * n[2] + x;
  return (int64_t)row * channels;
}

template <int VEC>
__global__ void __launch_bounds__(RS_THREADS) grid_resample_fwd(const RsGrid a) {
  RsLane l;
  if (!rs_lane<VEC>(a, a.dn, l)) return;
  const int32_t C = a.cgn * VEC;
  const RsTap tz = rs_tap(l.z, a.a[0], a.align, a.sn[0]);
  const RsTap ty = rs_tap(l.y, a.a[1], a.align, a.sn[1]);
  const RsTap tx = rs_tap(l.x, a.a[2], a.align, a.sn[2]);
  const int32_t iz[2] = {tz.i0, tz.i1}, iy[2] = {ty.i0, ty.i1}, ix[2] = {tx.i0, tx.i1};
  const float wz[2] = {tz.w0, tz.w1}, wy[2] = {ty.w0, ty.w1}, wx[2] = {tx.w0, tx.w1};
  Vec<VEC> v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k)
    v[k] = vec_load<VEC>(a.in + rs_elem(a.sn, l.b, iz[k >> 2], iy[(k >> 1) & 1], ix[k & 1], C) + l.c0);
  Vec<VEC> acc;
#pragma unroll
  for (int c = 0; c < VEC; ++c) acc.v[c] = 0.0f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float w = (wz[k >> 2] * wy[(k >> 1) & 1]) * wx[k & 1];
#pragma unroll
    for (int c = 0; c < VEC; ++c) acc.v[c] += w * v[k].v[c];
  }
  vec_store<VEC>(a.out + rs_elem(a.dn, l.b, l.z, l.y, l.x, C) + l.c0, acc);
}

// Outputs [lo, hi] of an axis whose taps touch input cell i (empty: lo > hi).  Candidates: src(o) within (i - 1, i + 1) inverted in
// fp32 -- widened by a quarter cell plus 2^-20 relative in input space and by 2 outputs plus 2^-20 relative in output space, which
// covers the rounding of the forward's src and of this inverse for every extent below 2^31 -- then narrowed by the taps themselves.
LP_DEV void rs_range(int32_t i, float a, float ia, int32_t align, int32_t n_in, int32_t n_out, int32_t& lo, int32_t& hi) {
  lo = 0, hi = n_out - 1;
  if (ia > 0.0f) {
    const float off = align ? 0.0f : 0.5f;
    const float d = 1.25f + (float)i * 9.5367431640625e-7f;
    if (i > 0) {
      const float x = fmaxf(((float)i - d + off) * ia - off, 0.0f);
      const float f = floorf(x - 2.0f - x * 9.5367431640625e-7f);
      if (f > 0.0f) lo = f >= (float)n_out ? n_out : (int32_t)f;
    }
    if (i < n_in - 1) {
      const float x = fmaxf(((float)i + d + off) * ia - off, 0.0f);
      const float f = ceilf(x + 2.0f + x * 9.5367431640625e-7f);
      if (f < (float)(n_out - 1)) hi = (int32_t)f;
    }
  }
  for (; lo <= hi; ++lo) {
    const RsTap t = rs_tap(lo, a, align, n_in);
    if (t.i0 == i || t.i1 == i) break;
  }
  for (; hi >= lo; --hi) {
    const RsTap t = rs_tap(hi, a, align, n_in);
    if (t.i0 == i || t.i1 == i) break;
  }
}

// weight of input cell i in output cell o of an axis: (1 - lambda) where i0 == i, lambda where i1 == i, both at a clamped border
LP_DEV float rs_weight(int32_t o, int32_t i, float a, int32_t align, int32_t n_in) {
  const RsTap t = rs_tap(o, a, align, n_in);
  return (t.i0 == i ? t.w0 : 0.0f) + (t.i1 == i ? t.w1 : 0.0f);
}

template <int VEC, bool ACC>
__global__ void __launch_bounds__(RS_THREADS) grid_resample_bwd(const RsGrid a) {
  RsLane l;
  if (!rs_lane<VEC>(a, a.sn, l)) return;
  const int32_t C = a.cgn * VEC;
  int32_t zlo, zhi, ylo, yhi, xlo, xhi;
  rs_range(l.z, a.a[0], a.ia[0], a.align, a.sn[0], a.dn[0], zlo, zhi);
  rs_range(l.y, a.a[1], a.ia[1], a.align, a.sn[1], a.dn[1], ylo, yhi);
  rs_range(l.x, a.a[2], a.ia[2], a.align, a.sn[2], a.dn[2], xlo, xhi);
  Vec<VEC> acc;
#pragma unroll
  for (int c = 0; c < VEC; ++c) acc.v[c] = 0.0f;
  for (int32_t oz = zlo; oz <= zhi; ++oz) {
    const float wz = rs_weight(oz, l.z, a.a[0], a.align, a.sn[0]);
    for (int32_t oy = ylo; oy <= yhi; ++oy) {
      const float wzy = wz * rs_weight(oy, l.y, a.a[1], a.align, a.sn[1]);
      const float* p = a.in + rs_elem(a.dn, l.b, oz, oy, xlo, C) + l.c0;
      for (int32_t ox = xlo; ox <= xhi; ++ox, p += C) {
        const float w = wzy * rs_weight(ox, l.x, a.a[2], a.align, a.sn[2]);
        const Vec<VEC> g = vec_load<VEC>(p);
#pragma unroll
        for (int c = 0; c < VEC; ++c) acc.v[c] += w * g.v[c];
      }
    }
  }
  float* po = a.out + rs_elem(a.sn, l.b, l.z, l.y, l.x, C) + l.c0;
  if (ACC) {
    const Vec<VEC> old = vec_load<VEC>(po);
#pragma unroll
    for (int c = 0; c < VEC; ++c) acc.v[c] = old.v[c] + acc.v[c];
  }
  vec_store<VEC>(po, acc);
}

// ---------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------

// The coefficient of one axis when the caller gives none: (n_in - 1) / (n_out - 1) (0 for n_out == 1) with align_corners, n_in / n_out
// without; fp32 division of the fp32 extents, as torch.nn.functional.interpolate derives it from sizes.
float grid_resample_coeff(int n_in, int n_out, bool align) {
  if (align) return n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.0f;
  return (float)n_in / (float)n_out;
}

// `src`, `dst` normalised (every grid carries its base pointer) and checked by lp_api.hip.  backward == false: dst = R src.
// backward == true: src (= | +=) R^T dst, i.e. `src` holds the gradient buffers of the source and `dst` the upstream gradient.
int grid_resample_launch(const LpGridList& src, const LpGridList& dst, int align, const float* coeffs, bool backward, bool accumulate,
                         hipStream_t stream) {
  const int C = src.channels;
  int vec = row_vec(C, {});
  for (int g = 0; g < src.n_grids && vec == 4; ++g) vec = row_vec(C, {src.grids[g].data, dst.grids[g].data});
  for (int g = 0; g < src.n_grids; ++g) {
    const LpGrid& s = src.grids[g];
    const LpGrid& d = dst.grids[g];
    RsGrid t;
    const float* ps = s.data + s.row_offset * C;
    const float* pd = d.data + d.row_offset * C;
    t.in = backward ? pd : ps;
    t.out = const_cast<float*>(backward ? ps : pd);
    t.B = s.B;
    t.sn[0] = s.D, t.sn[1] = s.H, t.sn[2] = s.W;
    t.dn[0] = d.D, t.dn[1] = d.H, t.dn[2] = d.W;
    for (int ax = 0; ax < 3; ++ax) {
      t.a[ax] = coeffs ? coeffs[3 * g + ax] : grid_resample_coeff(t.sn[ax], t.dn[ax], align != 0);
      t.ia[ax] = t.a[ax] > 0.0f ? (float)(1.0 / (double)t.a[ax]) : 0.0f;
    }
    t.align = align;
    t.cgn = C / vec;
    const int32_t* own = backward ? t.sn : t.dn;  // the side whose cells the lanes own
    const int64_t items = (int64_t)own[1] * own[2] * t.cgn;
    const int64_t tiles = (items + RS_THREADS - 1) / RS_THREADS;
    unsigned blocks;
    if (int rc = launch_blocks("lp_grid_resample", tiles * own[0] * (int64_t)t.B, 1, blocks)) return rc;
    t.tiles = (uint32_t)tiles;
    const dim3 gr(blocks), bl(RS_THREADS);
    if (!backward) {
      if (vec == 4) hipLaunchKernelGGL((grid_resample_fwd<4>), gr, bl, 0, stream, t);
      else hipLaunchKernelGGL((grid_resample_fwd<1>), gr, bl, 0, stream, t);
    } else if (accumulate) {
      if (vec == 4) hipLaunchKernelGGL((grid_resample_bwd<4, true>), gr, bl, 0, stream, t);
      else hipLaunchKernelGGL((grid_resample_bwd<1, true>), gr, bl, 0, stream, t);
    } else {
      if (vec == 4) hipLaunchKernelGGL((grid_resample_bwd<4, false>), gr, bl, 0, stream, t);
      else hipLaunchKernelGGL((grid_resample_bwd<1, false>), gr, bl, 0, stream, t);
    }
    const int rc = check_launch(backward ? "grid_resample_bwd" : "grid_resample_fwd");
    if (rc) return rc;
  }
  return LP_OK;
}

const char* build_info_grid_resample() {
  return "{\"modes\": [\"trilinear\", \"bilinear (planes)\"], \"row_loads\": \"16 bytes where C % 4 == 0, 4 bytes otherwise\", "
         "\"forward\": \"output-stationary, 8 taps per lane\", \"adjoint\": \"input-stationary gather, fixed order; no atomics\"}";
}

}  // namespace lp

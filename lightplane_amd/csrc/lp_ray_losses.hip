// lp_ray_losses.hip -- the distortion loss and the interlevel (proposal) loss of mip-NeRF 360 on the samples of the march in pieces
// (include/lightplane_hip_losses.h has the definitions).  fp32 in and out, no atomics, no workspace, no host synchronisation; the
// backwards recompute the scans from the inputs.  Arguments are checked by lp_api.hip.
//
// One wavefront (= one workgroup) per ray, lanes over samples in chunks of 64; a scan over the ray is a wave scan per chunk plus a
// carry, the sum of the chunks before it (after it, for the suffix scans, which walk the chunks from the far end).
//
// Distortion.  D_i = sum_{k < i} gap_k A_k and E_i = sum_{k >= i} gap_k R_{k+1} are scans of products of scans: for w >= 0 every term is
// non-negative and nothing cancels (the prefix of w d would lose the digits that mass far from d_0 needs).
//   forward   one prefix pass: A, D, the two sums; no LDS
//   backward  the prefix pass leaves A_i - w_i (the exclusive scan) and D_i in LDS, a suffix pass forms R and E and writes the gradients
// Interlevel.  n_k = #{proposal edges <= target edge k} by bisection (k = 0 .. S; 16 bits each), lo_k = max(0, n_k - 1),
// hi_k = min(P, n_{k+1}), bound_k = C^[hi_k] - C^[lo_k] with the proposal's prefix sums C^ in fp64.
//   forward   C^ and the depths of both sides to LDS, n, then lanes over the cells
//   backward  the same, then G = prefix sums of c_k (fp64) and lanes over the proposal: #{k : lo_k <= j} = #{k < S : n_k <= j + 1} and
//             #{k : hi_k <= j} = #{k < S : n_{k+1} <= j}, two bisections in n, and the difference of G between them
#include "lp_host.h"
#include "lp_wave.h"

namespace lp {

namespace {

// the value of the lane before / after, 0 at the end of the wave: an exclusive scan from an inclusive one without `inclusive - x`
LP_DEV float lane_before(float x, int lane) {
  const float y = __shfl_up(x, 1, 64);
  return lane > 0 ? y : 0.0f;
}
LP_DEV float lane_after(float x, int lane) {
  const float y = __shfl_down(x, 1, 64);
  return lane < 63 ? y : 0.0f;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// distortion
// ------------------------------------------------------------------------------------------------------------------------------------

struct DistArgs {
  const float *weights, *depths, *deltas, *g_loss;
  float *loss, *g_weights, *g_depths, *g_deltas;
  int S;
};

// sample s0 + lane of a ray (zeros beyond the ray's end) and its prefix sums
struct DistLane {
  float w, delta, gap;  // gap = d_{s+1} - d_s, 0 for the last sample
  float A_before;       // sum_{j < s} w_j
  float D;              // sum_{k < s} gap_k A_k
};

// chunk s0 of the prefix pass; cA / cD: the sums of w and of gap_k A_k over the chunks before it
LP_DEV DistLane dist_prefix(const float* w, const float* d, const float* delta, int s0, int S, int lane, float& cA, float& cD) {
  const int s = s0 + lane;
  DistLane o;
  o.w = s < S ? w[s] : 0.0f;
  o.delta = s < S ? delta[s] : 0.0f;
  o.gap = s + 1 < S ? d[s + 1] - d[s] : 0.0f;
  const float a = wave_scan(o.w, lane);
  o.A_before = cA + lane_before(a, lane);
  const float t = wave_scan(o.gap * (cA + a), lane);
  o.D = cD + lane_before(t, lane);
  cA += __shfl(a, 63, 64);
  cD += __shfl(t, 63, 64);
  return o;
}

__global__ __launch_bounds__(64) void distortion_fwd(DistArgs a) {
  const int S = a.S, lane = threadIdx.x;
  const int64_t r = blockIdx.x, base = r * S;
  float cA = 0.0f, cD = 0.0f, pairs = 0.0f, self = 0.0f;
  for (int s0 = 0; s0 < S; s0 += 64) {
    const DistLane q = dist_prefix(a.weights + base, a.depths + base, a.deltas + base, s0, S, lane, cA, cD);
    pairs += q.w * q.D;
    self += (q.w * q.w) * q.delta;
  }
  pairs = wave_sum(pairs), self = wave_sum(self);
  if (lane == 0) a.loss[r] = 2.0f * pairs + self / 3.0f;
}

// dynamic LDS: A_before[S] | D[S]
__global__ __launch_bounds__(64) void distortion_bwd(DistArgs a) {
  extern __shared__ float smem[];
  const int S = a.S, lane = threadIdx.x;
  float* A_before = smem;
  float* D = smem + S;
  const int64_t r = blockIdx.x, base = r * S;
  const float *w = a.weights + base, *d = a.depths + base, *delta = a.deltas + base;
  float cA = 0.0f, cD = 0.0f;
  for (int s0 = 0; s0 < S; s0 += 64) {
    const DistLane q = dist_prefix(w, d, delta, s0, S, lane, cA, cD);
    if (s0 + lane < S) A_before[s0 + lane] = q.A_before, D[s0 + lane] = q.D;
  }
  __syncthreads();
  const float g = a.g_loss ? a.g_loss[r] : 1.0f;
  float cR = 0.0f, cE = 0.0f;  // the sums of w and of gap_k R_{k+1} over the chunks after this one
  for (int s0 = (S - 1) & ~63; s0 >= 0; s0 -= 64) {
    const int s = s0 + lane;
    const float ws = s < S ? w[s] : 0.0f;
    const float gap = s + 1 < S ? d[s + 1] - d[s] : 0.0f;
    const float rs = wave_rscan(ws, lane);
    const float R_after = cR + lane_after(rs, lane);  // sum_{j > s} w_j
    const float u = wave_rscan(gap * R_after, lane);
    const float E = cE + u;
    cR += __shfl(rs, 0, 64);
    cE += __shfl(u, 0, 64);
    if (s < S) {
      if (a.g_weights) a.g_weights[base + s] = g * (2.0f * (D[s] + E) + (2.0f * (ws * delta[s])) / 3.0f);
      if (a.g_depths) a.g_depths[base + s] = g * (2.0f * ws * (A_before[s] - R_after));
      if (a.g_deltas) a.g_deltas[base + s] = g * ((ws * ws) / 3.0f);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// interlevel
// ------------------------------------------------------------------------------------------------------------------------------------

struct InterArgs {
  const float *weights, *depths, *p_weights, *p_depths, *g_loss;
  float *loss, *g_p_weights;
  int S, P;
  float eps;
};

// the number of the P + 1 cell edges over the non-decreasing dh[0 .. P) that are <= x
LP_DEV int edges_not_above(const float* dh, int P, float x) {
  int lo = 0, hi = P + 1;  // (the answer is in [lo, hi])
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (bin_edge(dh, mid, P) <= x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// the number of entries of the non-decreasing v[0 .. n) that are <= x
LP_DEV int count_not_above(const uint16_t* v, int n, int x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((int)v[mid] <= x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// a ray's LDS (doubles first): C^[P + 1] | G[S + 1] (backward only) | dh[P] | d[S] | n[S + 1] of 16 bits
struct InterLds {
  double *C, *G;
  float *dh, *d;
  uint16_t* n;
};
LP_DEV InterLds inter_lds(double* smem, int S, int P, bool backward) {
  InterLds m;
  m.C = smem;
  m.G = m.C + P + 1;
  m.dh = (float*)(m.G + (backward ? S + 1 : 0));
  m.d = m.dh + P;
  m.n = (uint16_t*)(m.d + S);
  return m;
}
size_t inter_lds_bytes(int S, int P, bool backward) {
  return sizeof(double) * (size_t)(P + 1 + (backward ? S + 1 : 0)) + sizeof(float) * (size_t)(P + S) + sizeof(uint16_t) * (size_t)(S + 1);
}

// C^, both depth rows and n of ray r
LP_DEV void inter_stage(const InterArgs& a, int64_t r, int lane, const InterLds& m) {
  const int S = a.S, P = a.P;
  const float *pw = a.p_weights + r * P, *pd = a.p_depths + r * P, *td = a.depths + r * S;
  double carry = 0.0;
  if (lane == 0) m.C[0] = 0.0;
  for (int j0 = 0; j0 < P; j0 += 64) {
    const int j = j0 + lane;
    const double incl = wave_scan(j < P ? (double)pw[j] : 0.0, lane);
    if (j < P) {
      m.C[j + 1] = carry + incl;
      m.dh[j] = pd[j];
    }
    carry += __shfl(incl, 63, 64);
  }
  for (int s = lane; s < S; s += 64) m.d[s] = td[s];
  __syncthreads();
  for (int k = lane; k <= S; k += 64) m.n[k] = (uint16_t)edges_not_above(m.dh, P, bin_edge(m.d, k, S));
  __syncthreads();
}

// max(0, w_k - bound_k) of cell k
LP_DEV double inter_excess(const InterLds& m, int k, int P, float w) {
  const int n0 = m.n[k], n1 = m.n[k + 1];
  const int lo = n0 > 0 ? n0 - 1 : 0, hi = n1 < P ? n1 : P;
  const double x = (double)w - (m.C[hi] - m.C[lo]);
  return x > 0.0 ? x : 0.0;  // (a NaN is not > 0)
}

__global__ __launch_bounds__(64) void interlevel_fwd(InterArgs a) {
  extern __shared__ double smem_d[];
  const int S = a.S, lane = threadIdx.x;
  const int64_t r = blockIdx.x;
  const InterLds m = inter_lds(smem_d, S, a.P, false);
  inter_stage(a, r, lane, m);
  const float* w = a.weights + r * S;
  double sum = 0.0;
  for (int k = lane; k < S; k += 64) {
    const float wk = w[k];
    const double x = inter_excess(m, k, a.P, wk);
    sum += x * x / ((double)wk + (double)a.eps);
  }
  sum = wave_scan(sum, lane);
  if (lane == 63) a.loss[r] = (float)sum;
}

__global__ __launch_bounds__(64) void interlevel_bwd(InterArgs a) {
  extern __shared__ double smem_d[];
  const int S = a.S, P = a.P, lane = threadIdx.x;
  const int64_t r = blockIdx.x;
  const InterLds m = inter_lds(smem_d, S, P, true);
  inter_stage(a, r, lane, m);
  const float* w = a.weights + r * S;
  double carry = 0.0;
  if (lane == 0) m.G[0] = 0.0;
  for (int k0 = 0; k0 < S; k0 += 64) {
    const int k = k0 + lane;
    double c = 0.0;
    if (k < S) {
      const float wk = w[k];
      c = -2.0 * inter_excess(m, k, P, wk) / ((double)wk + (double)a.eps);
    }
    const double incl = wave_scan(c, lane);
    if (k < S) m.G[k + 1] = carry + incl;
    carry += __shfl(incl, 63, 64);
  }
  __syncthreads();
  const double g = a.g_loss ? (double)a.g_loss[r] : 1.0;
  float* out = a.g_p_weights + r * P;
  for (int j = lane; j < P; j += 64) {
    const int touched = count_not_above(m.n, S, j + 1);  // cells with lo_k <= j
    const int passed = count_not_above(m.n + 1, S, j);   // cells with hi_k <= j
    out[j] = (float)(g * (m.G[touched] - m.G[passed]));
  }
}

}  // namespace

// `a` checked by lp_api.hip: n_rays > 0, 1 <= S <= 2048, n_rays * S < 2^31
int distortion_launch(const LpDistortionArgs& a, bool backward, hipStream_t stream) {
  DistArgs s;
  s.weights = a.weights, s.depths = a.depths, s.deltas = a.deltas, s.g_loss = a.grad_loss;
  s.loss = a.loss, s.g_weights = a.grad_weights, s.g_depths = a.grad_depths, s.g_deltas = a.grad_deltas;
  s.S = a.n_samples;
  if (backward && !s.g_weights && !s.g_depths && !s.g_deltas) return LP_OK;
  unsigned blocks;
  if (int rc = launch_blocks(backward ? "lp_distortion_backward" : "lp_distortion_forward", a.n_rays, 1, blocks)) return rc;
  if (backward) {
    // at most 2 * 2048 * 4 = 16 384 bytes
    hipLaunchKernelGGL(distortion_bwd, dim3(blocks), dim3(64), sizeof(float) * 2 * (size_t)s.S, stream, s);
    return check_launch("distortion_bwd");
  }
  hipLaunchKernelGGL(distortion_fwd, dim3(blocks), dim3(64), 0, stream, s);
  return check_launch("distortion_fwd");
}

// `a` checked by lp_api.hip: n_rays > 0, 2 <= S, P <= 2048, n_rays * max(S, P) < 2^31
int interlevel_launch(const LpInterlevelArgs& a, bool backward, hipStream_t stream) {
  InterArgs s;
  s.weights = a.weights, s.depths = a.depths, s.p_weights = a.proposal_weights, s.p_depths = a.proposal_depths, s.g_loss = a.grad_loss;
  s.loss = a.loss, s.g_p_weights = a.grad_proposal_weights;
  s.S = a.n_samples, s.P = a.n_proposal, s.eps = a.eps;
  unsigned blocks;
  if (int rc = launch_blocks(backward ? "lp_interlevel_backward" : "lp_interlevel_forward", a.n_rays, 1, blocks)) return rc;
  // at S = P = 2048: 8 * 2049 + 4 * 4096 + 2 * 2049 = 36 874 bytes forward, 8 * 2049 more = 53 266 backward: below the 64 KB a
  // workgroup has without asking
  const size_t lds = inter_lds_bytes(s.S, s.P, backward);
  if (backward) {
    hipLaunchKernelGGL(interlevel_bwd, dim3(blocks), dim3(64), lds, stream, s);
    return check_launch("interlevel_bwd");
  }
  hipLaunchKernelGGL(interlevel_fwd, dim3(blocks), dim3(64), lds, stream, s);
  return check_launch("interlevel_fwd");
}

}  // namespace lp

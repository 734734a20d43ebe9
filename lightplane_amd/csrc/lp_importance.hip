// lp_importance.hip -- importance resampling for the march in pieces (include/lightplane_hip_importance.h): N new depths per ray drawn
// from the histogram the compositing weights of a coarse march are, merged into the coarse depths, with their deltas and points.
// fp32, no atomics, no workspace, no host synchronisation.  Arguments are checked by lp_api.hip.
//
// Forward: one wavefront (= one workgroup) per ray, everything of the ray in LDS.  The stratified targets ascend, so the new depths
// come out sorted and the merge is a rank computation: a coarse sample goes to its index + the number of new depths below it, a new
// depth to its index + the number of coarse depths not above it -- two binary searches, no sort.
//   1  lanes over bins in chunks of 64: p = max(w, 0) + pad, inclusive wave scan with a carry between chunks -> C[0 .. S]; d[0 .. S)
//   2  lanes over k: binary search of u_k W in C, a from the two entries the search ended between, t[k] clamped to its bin's edges
//   3  ranks: every coarse and every new depth writes its slot of out[0 .. S')                        (include_coarse only)
//   4  depths' / deltas' one lane per sample; points' as the ray's contiguous run of 3 S' floats
// The bin edges are not kept: e_j = (d[j-1] + d[j]) / 2 is two LDS reads and an add where it is needed (twice per new depth).
#include "lp_host.h"
#include "lp_wave.h"

namespace lp {

namespace {

constexpr int IB_THREADS = 256;  // importance_bwd: 4 rays per workgroup

struct ImpArgs {
  const float *origins, *directions, *depths, *weights, *jitter;
  int64_t n_rays;
  int S, N, S_out;
  bool merge;
  float pad;
  float *points, *out_depths, *out_deltas;
  const float* g_points;
  float *g_origins, *g_directions;
};

// the number of entries of the non-decreasing v[0 .. n) that are < x (STRICT) or <= x
template <bool STRICT>
LP_DEV int count_below(const float* v, int n, float x) {
  int lo = 0, hi = n;  // (the answer is in [lo, hi])
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (STRICT ? v[mid] < x : v[mid] <= x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// dynamic LDS: C[S + 1] | d[S] | t[N] | out[S + N] (merge only; without it the results are t)
__global__ __launch_bounds__(64) void importance_fwd(ImpArgs a) {
  extern __shared__ float smem[];
  const int S = a.S, N = a.N, S_out = a.S_out;
  float* C = smem;
  float* d = C + S + 1;
  float* t = d + S;
  float* out = a.merge ? t + N : t;
  const int lane = threadIdx.x;
  const int64_t r = blockIdx.x;

  // ---- 1: histogram -> CDF ----
  const int64_t base = r * S;
  float carry = 0.0f;
  if (lane == 0) C[0] = 0.0f;
  for (int s0 = 0; s0 < S; s0 += 64) {
    const int s = s0 + lane;
    const bool in = s < S;
    const float w = in ? a.weights[base + s] : 0.0f;
    const float p = in ? (w > 0.0f ? w : 0.0f) + a.pad : 0.0f;  // (a NaN is not > 0)
    const float incl = wave_scan(p, lane);
    if (in) {
      C[s + 1] = carry + incl;
      d[s] = a.depths[base + s];
    }
    carry += __shfl(incl, 63, 64);
  }
  __syncthreads();

  // ---- 2: inverse CDF at the stratified targets ----
  const float W = C[S];
  for (int k = lane; k < N; k += 64) {
    const float xi = a.jitter ? a.jitter[r * N + k] : 0.5f;
    const float x = (((float)k + xi) / (float)N) * W;
    int lo = 0, hi = S - 1;  // the last bin j with C[j] <= x, in [lo, hi] (C[0] = 0)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (C[mid] <= x) lo = mid;
      else hi = mid - 1;
    }
    const float c0 = C[lo];
    const float den = C[lo + 1] - c0;
    float f = den > 0.0f ? (x - c0) / den : 0.0f;
    f = fminf(fmaxf(f, 0.0f), 1.0f);  // (and a NaN becomes 0)
    const float e0 = bin_edge(d, lo, S), e1 = bin_edge(d, lo + 1, S);
    t[k] = fminf(fmaxf(e0 + f * (e1 - e0), e0), e1);
  }
  __syncthreads();

  // ---- 3: merge by rank (ties: the coarse sample first) ----
  if (a.merge) {
    for (int s = lane; s < S; s += 64) {
      const float v = d[s];
      out[s + count_below<true>(t, N, v)] = v;
    }
    for (int k = lane; k < N; k += 64) {
      const float v = t[k];
      out[k + count_below<false>(d, S, v)] = v;
    }
    __syncthreads();
  }

  // ---- 4: results ----
  const int64_t obase = r * S_out;
  for (int i = lane; i < S_out; i += 64) {
    const float v = out[i];
    a.out_depths[obase + i] = v;
    a.out_deltas[obase + i] = i > 0 ? v - out[i - 1] : (S_out > 1 ? out[1] - v : 1.0f);
  }
  Ray q;
  load_ray_line(a.origins, a.directions, r, q);
  q.near_t = q.far_t = 0.0f;
  q.b = 0;
  float* pts = a.points + 3 * obase;
  for (int e = lane; e < 3 * S_out; e += 64) {
    const int i = e / 3, c = e - 3 * i;
    float x, y, z;
    sample_point(q, out[i], false, x, y, z);
    pts[e] = c == 0 ? x : c == 1 ? y : z;
  }
}

// One wavefront per ray: grad_points is read as the contiguous run of 3 S' floats it is (element e: sample e / 3, component e % 3).
__global__ __launch_bounds__(IB_THREADS) void importance_bwd(ImpArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * (IB_THREADS / 64) + (threadIdx.x >> 6);
  if (r >= a.n_rays) return;  // (wave-uniform)
  const int S_out = a.S_out;
  const float* gp = a.g_points + 3 * r * S_out;
  const float* dp = a.out_depths + r * S_out;
  float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f, d0 = 0.0f, d1 = 0.0f, d2 = 0.0f;
  for (int e = lane; e < 3 * S_out; e += 64) {
    const int i = e / 3, c = e - 3 * i;
    const float v = gp[e];
    const float vd = v * dp[i];
    o0 += c == 0 ? v : 0.0f;
    o1 += c == 1 ? v : 0.0f;
    o2 += c == 2 ? v : 0.0f;
    d0 += c == 0 ? vd : 0.0f;
    d1 += c == 1 ? vd : 0.0f;
    d2 += c == 2 ? vd : 0.0f;
  }
  o0 = wave_sum(o0), o1 = wave_sum(o1), o2 = wave_sum(o2);
  d0 = wave_sum(d0), d1 = wave_sum(d1), d2 = wave_sum(d2);
  if (lane == 0) {
    if (a.g_origins) a.g_origins[3 * r + 0] = o0, a.g_origins[3 * r + 1] = o1, a.g_origins[3 * r + 2] = o2;
    if (a.g_directions) a.g_directions[3 * r + 0] = d0, a.g_directions[3 * r + 1] = d1, a.g_directions[3 * r + 2] = d2;
  }
}

}  // namespace

// `a` checked by lp_api.hip: n_rays > 0, 2 <= S <= 2048, 1 <= N <= 2048, n_rays * (S + N) < 2^31
int importance_launch(const LpImportanceArgs& a, bool backward, hipStream_t stream) {
  ImpArgs s;
  s.origins = a.origins, s.directions = a.directions, s.depths = a.depths, s.weights = a.weights, s.jitter = a.jitter;
  s.n_rays = a.n_rays, s.S = a.n_samples, s.N = a.n_importance;
  s.merge = a.include_coarse != 0;
  s.S_out = s.merge ? s.S + s.N : s.N;
  s.pad = a.pad;
  s.points = a.out_points, s.out_depths = a.out_depths, s.out_deltas = a.out_deltas;
  s.g_points = a.grad_points, s.g_origins = a.grad_origins, s.g_directions = a.grad_directions;
  if (backward) {
    if (!s.g_origins && !s.g_directions) return LP_OK;
    unsigned blocks;
    if (int rc = launch_blocks("lp_importance_samples_backward", s.n_rays, IB_THREADS / 64, blocks)) return rc;
    hipLaunchKernelGGL(importance_bwd, dim3(blocks), dim3(IB_THREADS), 0, stream, s);
    return check_launch("importance_bwd");
  }
  // at most 4 * (2049 + 2048 + 2048 + 4096) = 40 964 bytes: below the 64 KB a workgroup has without asking
  const size_t lds = sizeof(float) * (size_t)(2 * s.S + 1 + s.N + (s.merge ? s.S + s.N : 0));
  // (one workgroup per ray: check_point_batch of lp_api.hip keeps n_rays * (S + N), hence n_rays, below 2^31)
  hipLaunchKernelGGL(importance_fwd, dim3((unsigned)s.n_rays), dim3(64), lds, stream, s);
  return check_launch("importance_fwd");
}

}  // namespace lp

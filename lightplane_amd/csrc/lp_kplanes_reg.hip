// lp_kplanes_reg.hip -- the three regularisers of a K-Planes field on the plane layout: values, gradient, or both in one sweep.
//
// Plane j of scale s is X[b, i_v, i_u, c] = planes[b, offset[s][j] + i_u + n_u * i_v, c] (lightplane_hip_kplanes_reg.h):
//   space_tv        first differences along u on every plane and along v on xy / xz / yz, phi_p(d), p in {1, 2};
//   time_smoothness on xt / yt / zt: s_k^2 with s_k = X[k + 1] - 2 X[k] + X[k - 1], 1 <= k <= n_v - 2;
//                   d / d X[k] = 2 / N * (s_{k - 1} - 2 s_k + s_{k + 1}) -- a 5-point stencil along v (s of a k outside the range is 0);
//   time_l1         on xt / yt / zt: |1 - X|, derivative sign(X - 1), 0 at X == 1.
// Every term is a mean per (plane, axis), summed over planes and scales.
//
// Traversal: ONE launch for all batch elements, scales and planes.  The host turns the layout into a table of at
// most 48 plane descriptors that travels by value; a workgroup finds its (batch element, plane, strip of u, chunk of i_v) from the
// prefix of the planes' workgroup counts.  The 256 lanes of a workgroup cover the (i_u, float4 of channels) positions of a strip of
// 256 / (C / 4) vertices -- one coalesced 4 KB run per row -- and march KR_VC rows along i_v, the slow axis, carrying the rows of the
// v-stencil in registers (3 on a space plane, 5 on a space-time plane), so a row is fetched once per chunk plus the chunk's halo rows.
// The u-neighbours, C / 4 lanes away and in another wavefront for wide rows, come from an LDS copy of the current row; the strip's
// two halo vertices are the only re-reads along u.  Loads run one row ahead of their use.
//
// Reduction, in a fixed order (no atomics in this file): a lane sums each term in fp32 over its <= KR_VC rows; the three sums, scaled
// in fp64 by 1 / pairs, go through the wave (wave_scan, lp_wave.h) and the workgroup in fp64, and the workgroup writes ONE double[3]
// into the workspace; kplanes_reg_finish (one workgroup) sums the partials in fp64 and writes the three fp32 terms.  The gradient is
// in gather form: every element is computed from its stencil and stored once with a vector store (or read-add-store).
#include "lp_host.h"
#include "lp_rows.h"
#include "lp_wave.h"

namespace lp {

constexpr int KR_THREADS = 256;
constexpr int KR_VC = 32;         // rows of i_v a workgroup marches: the halo rows are 2 / 32 (space) or 4 / 32 (space-time) of its reads
constexpr int KR_MAX_PLANES = LP_KPLANES_MAX_SCALES * LP_KPLANES_MAX_PLANES;
constexpr int KR_MAX_LPV = 16;    // lanes per vertex at C = 64

struct RegPlane {
  int64_t row0;        // first row of the plane
  int32_t n_u, n_v;
  uint32_t strips;     // ceil(n_u / (KR_THREADS / lpv))
  uint32_t end;        // workgroups of one batch element up to and including this plane (strips * chunks each)
  int32_t is_time;     // xt / yt / zt: v is the time axis
  float cf[3];         // 1 / pairs -- space plane: TV along u, TV along v, unused; space-time plane: TV along u, smoothness, l1
  double cd[3];        // the same in fp64 (terms)
};

struct RegSweep {
  const float* x;
  float* g;                 // gradient, same layout (NULL without GRAD)
  const float* grad_terms;  // device [3] or NULL (= 1, 1, 1) ...
  float weights[3];         // ... times these: the factors of the stored gradient
  double* partials;         // [workgroups][3]
  int64_t rows;             // per batch element
  int32_t lpv;              // lanes per vertex: C / 4
  int32_t n_planes;
  uint32_t per_batch;       // workgroups per batch element
  RegPlane plane[KR_MAX_PLANES];
};

template <int P>
LP_DEV float reg_phi(float d) {
  return P == 1 ? fabsf(d) : d * d;
}
template <int P>
LP_DEV float reg_dphi(float d) {
  return P == 1 ? (float)(d > 0.0f) - (float)(d < 0.0f) : 2.0f * d;
}

// (a row position in LDS is one 16-byte word)
LP_DEV float4 reg_f4(const Vec<4>& r) { return make_float4(r.v[0], r.v[1], r.v[2], r.v[3]); }
LP_DEV Vec<4> reg_vec(const float4& f) { return Vec<4>{{f.x, f.y, f.z, f.w}}; }

// (workgroup sum in fp64, fixed order; every thread of the workgroup calls it; valid in thread 0)
LP_DEV double reg_block_sum(double v, double* wave_part) {
  const int lane = threadIdx.x & 63;
  v = wave_scan<double>(v, lane);  // lane 63: the wave's sum
  __syncthreads();                 // (the slots of the call before have been read)
  if (lane == 63) wave_part[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < KR_THREADS / 64; ++w) s += wave_part[w];
  }
  return s;
}

// One workgroup's march over rows [k0, k1) of its strip.  TIME: a space-time plane (v-stencil of 5 rows with GRAD, 3 without);
// otherwise a space plane (3 rows with GRAD, 2 without).  win[2] is row k; win[2 - i] / win[2 + i] are rows k -+ i where the stencil
// needs them and they exist, and are never read otherwise.
template <int P, bool TIME, bool LOSS, bool GRAD, bool ACC>
LP_DEV void reg_march(const RegSweep& a, const RegPlane& pl, int b, int strip, int k0, float4 (*row)[KR_THREADS + 2 * KR_MAX_LPV],
                      const float g[3], float sum[3]) {
  constexpr int AHEAD = (TIME && GRAD) ? 2 : 1;            // rows after k the stencil reads
  constexpr int BEHIND = GRAD ? AHEAD : (TIME ? 1 : 0);    // rows before k
  const int t = threadIdx.x;
  const int lpv = a.lpv;
  const int su = KR_THREADS / lpv;  // vertices of a strip
  const int u0 = strip * su;
  const int u = u0 + t / lpv;
  const int n_u = pl.n_u, n_v = pl.n_v;
  const int k1 = min(k0 + KR_VC, n_v);
  const bool active = u < n_u;
  const bool has_um = active && u > 0, has_up = active && u + 1 < n_u;
  // the halo vertices of the strip: lanes [0, lpv) fetch vertex u0 - 1, lanes [lpv, 2 lpv) vertex u0 + su, where they exist
  const bool halo_l = GRAD && t < lpv && u0 > 0;  // (the values need the right neighbour only)
  const bool halo_r = t >= lpv && t < 2 * lpv && u0 + su < n_u;
  const bool halo = halo_l || halo_r;
  const int64_t sv = (int64_t)n_u * lpv * 4;  // floats to the next i_v row
  const int64_t plane0 = ((int64_t)b * a.rows + pl.row0) * lpv * 4;
  // (an inactive lane and a lane without halo duty get offsets they never use)
  const int64_t own = plane0 + ((int64_t)u * lpv + t % lpv) * 4;
  const int64_t hal = plane0 + ((int64_t)(halo_l ? u0 - 1 : u0 + su) * lpv + t % lpv) * 4;
  const int hslot = halo_l ? t : KR_THREADS + t;  // [0, lpv): left halo; [lpv + 256, 2 lpv + 256): right halo

  const Vec<4> zero = {{0.0f, 0.0f, 0.0f, 0.0f}};
  Vec<4> win[5] = {zero, zero, zero, zero, zero};
  Vec<4> hcur = zero;
  if (active) {
#pragma unroll
    for (int i = -BEHIND; i <= AHEAD; ++i)
      if (k0 + i >= 0 && k0 + i < n_v) win[2 + i] = vec_load<4>(a.x + own + (k0 + i) * sv);
  }
  if (halo) hcur = vec_load<4>(a.x + hal + k0 * sv);

  for (int k = k0; k < k1; ++k) {
    // the loads of the next step, issued before this step's arithmetic
    Vec<4> nxt = zero, hnxt = zero;
    const bool more = k + 1 < k1;
    if (active && more && k + 1 + AHEAD < n_v) nxt = vec_load<4>(a.x + own + (k + 1 + AHEAD) * sv);
    if (halo && more) hnxt = vec_load<4>(a.x + hal + (k + 1) * sv);

    // the current row with its two halo vertices in LDS, double-buffered: one barrier per row
    float4* cur = row[k & 1];
    cur[lpv + t] = reg_f4(win[2]);
    if (halo) cur[hslot] = reg_f4(hcur);
    __syncthreads();
    if (active) {
      const Vec<4> x0 = win[2];
      const Vec<4> xp = has_up ? reg_vec(cur[t + 2 * lpv]) : x0;  // a missing neighbour is the vertex itself: difference 0, phi(0) = phi'(0) = 0
      const Vec<4> xm = (GRAD && has_um) ? reg_vec(cur[t]) : x0;
      const bool v_m = k > 0, v_p = k + 1 < n_v;                             // (space) the pairs (k - 1, k) and (k, k + 1) exist
      const bool s_m = k >= 2 && k + 1 <= n_v, s_0 = k >= 1 && k + 2 <= n_v, s_p = k + 3 <= n_v;  // (space-time) triples centred at k - 1, k, k + 1
      Vec<4> out;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float x = x0.v[c];
        const float du = xp.v[c] - x;
        float gu = 0.0f, g1 = 0.0f, g2 = 0.0f;
        if (LOSS) sum[0] += reg_phi<P>(du);
        if (GRAD) gu = reg_dphi<P>(x - xm.v[c]) - reg_dphi<P>(du);
        if (TIME) {
          const float sc = s_0 ? (win[3].v[c] - 2.0f * x) + win[1].v[c] : 0.0f;
          const float e = 1.0f - x;
          if (LOSS) {
            sum[1] += sc * sc;
            sum[2] += fabsf(e);
          }
          if (GRAD) {
            const float sa = s_m ? (x - 2.0f * win[1].v[c]) + win[0].v[c] : 0.0f;
            const float sb = s_p ? (win[4].v[c] - 2.0f * win[3].v[c]) + x : 0.0f;
            g1 = 2.0f * ((sa - 2.0f * sc) + sb);
            g2 = (float)(e < 0.0f) - (float)(e > 0.0f);
            out.v[c] = g[0] * (pl.cf[0] * gu) + g[1] * (pl.cf[1] * g1) + g[2] * (pl.cf[2] * g2);
          }
        } else {
          const float dv = v_p ? win[3].v[c] - x : 0.0f;
          if (LOSS) sum[1] += reg_phi<P>(dv);
          if (GRAD) {
            g1 = reg_dphi<P>(v_m ? x - win[1].v[c] : 0.0f) - reg_dphi<P>(dv);
            out.v[c] = g[0] * (pl.cf[0] * gu + pl.cf[1] * g1);
          }
        }
      }
      if (GRAD) {
        float* pg = a.g + own + k * sv;
        if (ACC) {
          const Vec<4> old = vec_load<4>(pg);
#pragma unroll
          for (int c = 0; c < 4; ++c) out.v[c] = old.v[c] + out.v[c];
        }
        vec_store<4>(pg, out);
      }
    }
    win[0] = win[1], win[1] = win[2], win[2] = win[3];
    if (AHEAD == 2) win[3] = win[4], win[4] = nxt;
    else win[3] = nxt;
    hcur = hnxt;
  }
}

template <int P, bool LOSS, bool GRAD, bool ACC>
__global__ void __launch_bounds__(KR_THREADS) kplanes_reg_sweep(const RegSweep a) {
  __shared__ float4 row[2][KR_THREADS + 2 * KR_MAX_LPV];
  __shared__ double wave_part[KR_THREADS / 64];
  const uint32_t bid = blockIdx.x;
  const int b = (int)(bid / a.per_batch);
  const uint32_t r = bid % a.per_batch;
  int j = 0;
  while (j + 1 < a.n_planes && r >= a.plane[j].end) ++j;  // (uniform: scalar loads of the table)
  const RegPlane& pl = a.plane[j];
  const uint32_t in_plane = r - (j ? a.plane[j - 1].end : 0u);
  // strip fastest: the workgroups resident together march the same chunk of rows
  const int strip = (int)(in_plane % pl.strips);
  const int k0 = (int)(in_plane / pl.strips) * KR_VC;
  float g[3] = {0.0f, 0.0f, 0.0f};
  if (GRAD) {
#pragma unroll
    for (int i = 0; i < 3; ++i) g[i] = a.weights[i] * (a.grad_terms ? a.grad_terms[i] : 1.0f);
  }
  float sum[3] = {0.0f, 0.0f, 0.0f};
  if (pl.is_time) reg_march<P, true, LOSS, GRAD, ACC>(a, pl, b, strip, k0, row, g, sum);
  else reg_march<P, false, LOSS, GRAD, ACC>(a, pl, b, strip, k0, row, g, sum);
  if (LOSS) {
    // space plane: both sums are space_tv; space-time plane: TV along u, smoothness, l1
    const double su = pl.cd[0] * (double)sum[0], sv = pl.cd[1] * (double)sum[1], sl = pl.cd[2] * (double)sum[2];
    const double term[3] = {pl.is_time ? su : su + sv, pl.is_time ? sv : 0.0, pl.is_time ? sl : 0.0};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double total = reg_block_sum(term[i], wave_part);
      if (threadIdx.x == 0) a.partials[(int64_t)bid * 3 + i] = total;
    }
  }
}

// terms[i] = fp32(sum of the n workgroup partials of term i), summed in fp64 in a fixed order by one workgroup
__global__ void __launch_bounds__(KR_THREADS) kplanes_reg_finish(const double* partials, int64_t n, float* terms) {
  __shared__ double wave_part[KR_THREADS / 64];
  for (int i = 0; i < 3; ++i) {
    double s = 0.0;
    for (int64_t w = threadIdx.x; w < n; w += KR_THREADS) s += partials[w * 3 + i];
    const double total = reg_block_sum(s, wave_part);
    if (threadIdx.x == 0) terms[i] = (float)total;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------

// the plane table of a checked layout; returns the workgroups per batch element
static int64_t reg_table(const LpKPlanesRegArgs& a, RegSweep* t) {
  const int lpv = a.channels / 4;
  const int su = KR_THREADS / lpv;
  int64_t end = 0;
  int n = 0;
  for (int s = 0; s < a.n_scales; ++s) {
    for (int j = 0; j < a.n_planes; ++j, ++n) {
      const int n_u = a.spatial[s], n_v = j < 3 ? a.spatial[s] : a.temporal[s];
      const int64_t strips = (n_u + su - 1) / su, chunks = (n_v + KR_VC - 1) / KR_VC;
      end += strips * chunks;
      if (!t) continue;
      RegPlane& pl = t->plane[n];
      pl.row0 = a.offset[s][j];
      pl.n_u = n_u, pl.n_v = n_v;
      pl.strips = (uint32_t)strips;
      pl.end = (uint32_t)end;
      pl.is_time = j >= 3;
      // elements per row of pairs: every batch element and channel
      const double per = (double)a.batch * a.channels;
      const double pairs_u = per * n_v * (n_u - 1);
      const double pairs[3] = {pairs_u, pl.is_time ? per * n_u * (n_v - 2) : per * n_u * (n_v - 1), pl.is_time ? per * n_u * n_v : 0.0};
      for (int i = 0; i < 3; ++i) {
        pl.cd[i] = pairs[i] > 0.0 ? 1.0 / pairs[i] : 0.0;  // (no triple at n_v == 2: the term is 0, not 0 / 0)
        pl.cf[i] = (float)pl.cd[i];
      }
    }
  }
  if (t) t->n_planes = n, t->per_batch = (uint32_t)end;
  return end;  // (<= 48 * 256 * 128 < 2^31)
}

int64_t kplanes_reg_workgroups(const LpKPlanesRegArgs& a) { return reg_table(a, nullptr) * a.batch; }

template <int P>
static void reg_launch(const RegSweep& t, unsigned blocks, bool loss, bool grad, bool acc, hipStream_t stream) {
  const dim3 gr(blocks), bl(KR_THREADS);
  if (loss && grad) {
    if (acc) hipLaunchKernelGGL((kplanes_reg_sweep<P, true, true, true>), gr, bl, 0, stream, t);
    else hipLaunchKernelGGL((kplanes_reg_sweep<P, true, true, false>), gr, bl, 0, stream, t);
  } else if (loss) {
    hipLaunchKernelGGL((kplanes_reg_sweep<P, true, false, false>), gr, bl, 0, stream, t);
  } else if (acc) {
    hipLaunchKernelGGL((kplanes_reg_sweep<P, false, true, true>), gr, bl, 0, stream, t);
  } else {
    hipLaunchKernelGGL((kplanes_reg_sweep<P, false, true, false>), gr, bl, 0, stream, t);
  }
}

// Arguments were checked by lp_api.hip.  workspace != NULL: the terms; want_grad: the gradient.
int kplanes_reg_launch(const LpKPlanesRegArgs& a, double* workspace, bool want_grad, hipStream_t stream) {
  const bool want_loss = workspace != nullptr;
  RegSweep t;
  t.x = a.planes;
  t.g = want_grad ? a.grad_planes : nullptr;
  t.grad_terms = a.grad_terms;
  for (int i = 0; i < 3; ++i) t.weights[i] = a.weights[i];
  t.partials = workspace;
  t.rows = a.rows;
  t.lpv = a.channels / 4;
  const int64_t per_batch = reg_table(a, &t);
  unsigned blocks;
  if (int rc = launch_blocks("lp_kplanes_reg", per_batch * a.batch, 1, blocks)) return rc;
  if (a.p == 1) reg_launch<1>(t, blocks, want_loss, want_grad, a.accumulate != 0, stream);
  else reg_launch<2>(t, blocks, want_loss, want_grad, a.accumulate != 0, stream);
  if (int rc = check_launch("kplanes_reg_sweep")) return rc;
  if (want_loss) {
    hipLaunchKernelGGL(kplanes_reg_finish, dim3(1), dim3(KR_THREADS), 0, stream, workspace, (int64_t)blocks, a.terms);
    return check_launch("kplanes_reg_finish");
  }
  return LP_OK;
}

const char* build_info_kplanes_reg() {
  return "{\"terms\": [\"space_tv\", \"time_smoothness\", \"time_l1\"], \"p\": [1, 2], \"row_loads\": \"16 bytes\", "
         "\"strip_lanes\": 256, \"row_chunk\": 32, \"launches\": \"one sweep for all scenes, scales and planes + one finish\", "
         "\"reduction\": \"fp32 per lane, fp64 per wave, workgroup and field; no atomics\"}";
}

}  // namespace lp

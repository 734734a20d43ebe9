// lp_grid_tv.hip -- total-variation regulariser of a grid-list: loss value, gradient, or both in one sweep.
//
// For one grid x [B, D, H, W, C] and p in {1, 2} (phi_1(d) = |d|, phi_2(d) = d^2):
//   T_a  = sum over adjacent pairs along spatial axis a (all B, all C) of phi_p(x[.., i + 1, ..] - x[.., i, ..]),  N_a = pairs
//   loss = sum_g w_g * sum_{a: n_a > 1} T_a / N_a
//   d loss / d x[i] = sum_a (w_g / N_a) * (phi'(x[i] - x[i - 1]) - phi'(x[i + 1] - x[i])), boundary terms dropped; phi_1'(0) = 0.
//
// Traversal: ONE kernel template does all three jobs.  A lane owns one (y, x, channel group) position of a
// z-slice and marches TV_ZC slices along D, carrying x[z - 1] and x[z] in registers and loading x[z + 1] -- the D-neighbour, which is
// H * W * C * 4 bytes away (8 MB for 256^2 x 32), is never fetched a second time.  The 256 lanes of a workgroup cover 256
// consecutive 16-byte groups of the slice (4 KB, fully coalesced); the W-neighbours (+-C floats) lie in the same 4 KB except at the
// tile's two ends (L1), the H-neighbours (+-W * C floats) are the tile another workgroup of the same z-chunk reads as its own at
// the same step (L2 / Infinity Cache).  Workgroups are numbered tile-fastest, so the resident ones march one z-chunk together.
//
// Reduction, in a fixed order (no atomics anywhere in this file): a lane sums phi per axis in fp32 over its <= TV_ZC steps, combines
// the three axes with the fp64 coefficients w_g / N_a, the wave and then the workgroup reduce in fp64 through shuffles and LDS, and
// the workgroup writes ONE fp64 partial into the workspace; grid_tv_finish (one workgroup) sums the partials in fp64 and writes the
// fp32 scalar.  The gradient is in gather form: every element is computed from its six neighbours and stored once with a vector
// store (overwrite, or read-add-store for the accumulate mode) -- bit-reproducible.
#include "lp_host.h"
#include "lp_rows.h"

namespace lp {

constexpr int TV_THREADS = 256;
constexpr int TV_ZC = 16;  // slices a lane marches: the chunk's first step re-reads its z - 1 / z neighbours (1 / 16 of the reads)

struct TvGrid {
  const float* x;  // first cell of the grid
  float* g;        // its gradient (same layout), NULL in the forward
  int32_t B, D, H, W;
  int32_t cgn;     // lane positions per cell: C / VEC
  uint32_t tiles;  // ceil(H * W * cgn / TV_THREADS)
  uint32_t nzc;    // ceil(D / TV_ZC)
  float cf[3];     // w_g / N_a for a = W, H, D (0 for a singleton axis)
  double cd[3];    // the same in fp64 (loss)
  const float* grad_loss;  // device scalar (NULL = 1) ...
  float scale;             // ... times this: the factor of the stored gradient
  double* partials;        // one per workgroup of this launch
};

template <int P>
LP_DEV float tv_phi(float d) {
  return P == 1 ? fabsf(d) : d * d;
}
template <int P>
LP_DEV float tv_dphi(float d) {
  return P == 1 ? (float)(d > 0.0f) - (float)(d < 0.0f) : 2.0f * d;
}

// (workgroup sum in fp64, fixed order; every thread of the workgroup calls it)
LP_DEV double tv_block_sum(double v) {
  __shared__ double wave_sum[TV_THREADS / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < TV_THREADS / 64; ++w) s += wave_sum[w];
  }
  return s;  // valid in thread 0
}

template <int P, int VEC, bool LOSS, bool GRAD, bool ACC>
__global__ void __launch_bounds__(TV_THREADS) grid_tv_sweep(const TvGrid a) {
  const uint32_t bid = blockIdx.x;
  const uint32_t tile = bid % a.tiles;
  const uint32_t rest = bid / a.tiles;
  const uint32_t zc = rest % a.nzc;
  const uint32_t b = rest / a.nzc;
  const int64_t items = (int64_t)a.H * a.W * a.cgn;  // lane positions per slice
  const int64_t j = (int64_t)tile * TV_THREADS + threadIdx.x;
  const bool active = j < items;
  float sum[3] = {0.0f, 0.0f, 0.0f};
  if (active) {
    const int64_t cell = j / a.cgn;  // y * W + x
    const int32_t xw = (int32_t)(cell % a.W), yh = (int32_t)(cell / a.W);
    const int64_t sx = (int64_t)a.cgn * VEC;  // floats to the W-neighbour (= C)
    const int64_t sy = sx * a.W, sz = sy * a.H;
    const bool has_xm = xw > 0, has_xp = xw + 1 < a.W, has_ym = yh > 0, has_yp = yh + 1 < a.H;
    const int32_t z0 = (int32_t)zc * TV_ZC;
    const int32_t z1 = min(z0 + TV_ZC, a.D);
    const int64_t off0 = ((int64_t)b * a.D + z0) * sz + j * VEC;
    const float* px = a.x + off0;
    float s = 1.0f;
    if (GRAD) s = a.scale * (a.grad_loss ? *a.grad_loss : 1.0f);
    Vec<VEC> cur = vec_load<VEC>(px);
    Vec<VEC> prev = cur;  // a missing neighbour is the cell itself: its difference is 0, and phi(0) = phi'(0) = 0
    if (GRAD && z0 > 0) prev = vec_load<VEC>(px - sz);
    for (int32_t z = z0; z < z1; ++z, px += sz) {
      const Vec<VEC> nxt = z + 1 < a.D ? vec_load<VEC>(px + sz) : cur;
      const Vec<VEC> xp = has_xp ? vec_load<VEC>(px + sx) : cur;
      const Vec<VEC> yp = has_yp ? vec_load<VEC>(px + sy) : cur;
      Vec<VEC> xm = cur, ym = cur;
      if (GRAD) {
        if (has_xm) xm = vec_load<VEC>(px - sx);
        if (has_ym) ym = vec_load<VEC>(px - sy);
      }
      Vec<VEC> out;
#pragma unroll
      for (int c = 0; c < VEC; ++c) {
        const float dw = xp.v[c] - cur.v[c], dh = yp.v[c] - cur.v[c], dd = nxt.v[c] - cur.v[c];
        if (LOSS) {
          sum[0] += tv_phi<P>(dw);
          sum[1] += tv_phi<P>(dh);
          sum[2] += tv_phi<P>(dd);
        }
        if (GRAD) {
          const float gw = tv_dphi<P>(cur.v[c] - xm.v[c]) - tv_dphi<P>(dw);
          const float gh = tv_dphi<P>(cur.v[c] - ym.v[c]) - tv_dphi<P>(dh);
          const float gd = tv_dphi<P>(cur.v[c] - prev.v[c]) - tv_dphi<P>(dd);
          out.v[c] = s * (a.cf[0] * gw + a.cf[1] * gh + a.cf[2] * gd);
        }
      }
      if (GRAD) {
        float* pg = a.g + (px - a.x);
        if (ACC) {
          const Vec<VEC> old = vec_load<VEC>(pg);
#pragma unroll
          for (int c = 0; c < VEC; ++c) out.v[c] = old.v[c] + out.v[c];
        }
        vec_store<VEC>(pg, out);
      }
      prev = cur;
      cur = nxt;
    }
  }
  if (LOSS) {
    const double part = a.cd[0] * (double)sum[0] + a.cd[1] * (double)sum[1] + a.cd[2] * (double)sum[2];
    const double total = tv_block_sum(part);
    if (threadIdx.x == 0) a.partials[bid] = total;
  }
}

// loss = fp32(sum of the n workgroup partials), summed in fp64 in a fixed order by one workgroup
__global__ void __launch_bounds__(TV_THREADS) grid_tv_finish(const double* partials, int64_t n, float* loss) {
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += TV_THREADS) s += partials[i];
  const double total = tv_block_sum(s);
  if (threadIdx.x == 0) *loss = (float)total;
}

// ---------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------

static inline int64_t tv_grid_blocks(const LpGrid& d, int channels, int vec) {
  const int64_t items = (int64_t)d.H * d.W * (channels / vec);
  const int64_t tiles = (items + TV_THREADS - 1) / TV_THREADS;
  const int64_t nzc = (d.D + TV_ZC - 1) / TV_ZC;
  return (int64_t)d.B * nzc * tiles;
}

// Workgroups of the sweep over the whole list = fp64 partials in the workspace.  The count depends on the channel count only through
// C / 4 (C % 4 == 0) or C: a list whose pointers turn out not to be 16-byte aligned runs the scalar path, which needs more -- so the
// query sizes for the scalar path's count whenever that is larger (it always is).
int64_t grid_tv_blocks(const LpGridList& gl, int vec) {
  int64_t n = 0;
  for (int g = 0; g < gl.n_grids; ++g) n += tv_grid_blocks(gl.grids[g], gl.channels, vec);
  return n;
}

int64_t grid_tv_workspace_bytes(const LpGridList& gl) { return grid_tv_blocks(gl, 1) * (int64_t)sizeof(double); }

template <int P, int VEC>
static void tv_launch(const TvGrid& t, unsigned blocks, bool loss, bool grad, bool acc, hipStream_t stream) {
  const dim3 gr(blocks), bl(TV_THREADS);
  if (loss && grad) {  // the fused sweep always accumulates
    hipLaunchKernelGGL((grid_tv_sweep<P, VEC, true, true, true>), gr, bl, 0, stream, t);
  } else if (loss) {
    hipLaunchKernelGGL((grid_tv_sweep<P, VEC, true, false, false>), gr, bl, 0, stream, t);
  } else if (acc) {
    hipLaunchKernelGGL((grid_tv_sweep<P, VEC, false, true, true>), gr, bl, 0, stream, t);
  } else {
    hipLaunchKernelGGL((grid_tv_sweep<P, VEC, false, true, false>), gr, bl, 0, stream, t);
  }
}

// `gl` normalised (every grid carries its base pointer); grads[g] = the gradient tensor mirroring the tensor grids[g].data points to
// (NULL entries: no gradient); weights: host array of n_grids floats or NULL (all 1).  Arguments were checked by lp_api.hip.
int grid_tv_launch(const LpGridList& gl, const float* weights, int p, float* loss, double* workspace, const float* grad_loss,
                   float scale, float* const* grads, bool accumulate, hipStream_t stream) {
  const bool want_loss = loss != nullptr, want_grad = grads != nullptr;
  const int C = gl.channels;
  int vec = row_vec(C, {});
  for (int g = 0; g < gl.n_grids && vec == 4; ++g) vec = row_vec(C, {gl.grids[g].data, want_grad ? grads[g] : nullptr});
  int64_t done = 0;
  for (int g = 0; g < gl.n_grids; ++g) {
    const LpGrid& d = gl.grids[g];
    TvGrid t;
    t.x = d.data + d.row_offset * C;
    t.g = want_grad ? grads[g] + d.row_offset * C : nullptr;
    t.B = d.B, t.D = d.D, t.H = d.H, t.W = d.W;
    t.cgn = C / vec;
    const int64_t items = (int64_t)d.H * d.W * t.cgn;
    t.tiles = (uint32_t)((items + TV_THREADS - 1) / TV_THREADS);
    t.nzc = (uint32_t)((d.D + TV_ZC - 1) / TV_ZC);
    const double w = weights ? (double)weights[g] : 1.0;
    const double cells = (double)d.B * d.D * d.H * d.W * C;
    const int n_axis[3] = {d.W, d.H, d.D};
    for (int a = 0; a < 3; ++a) {
      // pairs along the axis: every cell but the last of each line
      const double pairs = n_axis[a] > 1 ? cells / n_axis[a] * (n_axis[a] - 1) : 0.0;
      t.cd[a] = pairs > 0.0 ? w / pairs : 0.0;
      t.cf[a] = (float)t.cd[a];
    }
    t.grad_loss = grad_loss;
    t.scale = scale;
    t.partials = want_loss ? workspace + done : nullptr;
    unsigned blocks;
    if (int rc = launch_blocks("lp_grid_tv", tv_grid_blocks(d, C, vec), 1, blocks)) return rc;
    if (p == 1) {
      if (vec == 4) tv_launch<1, 4>(t, blocks, want_loss, want_grad, accumulate, stream);
      else tv_launch<1, 1>(t, blocks, want_loss, want_grad, accumulate, stream);
    } else {
      if (vec == 4) tv_launch<2, 4>(t, blocks, want_loss, want_grad, accumulate, stream);
      else tv_launch<2, 1>(t, blocks, want_loss, want_grad, accumulate, stream);
    }
    const int rc = check_launch("grid_tv_sweep");
    if (rc) return rc;
    done += blocks;
  }
  if (want_loss) {
    hipLaunchKernelGGL(grid_tv_finish, dim3(1), dim3(TV_THREADS), 0, stream, workspace, done, loss);
    return check_launch("grid_tv_finish");
  }
  return LP_OK;
}

const char* build_info_grid_tv() {
  return "{\"p\": [1, 2], \"row_loads\": \"16 bytes where C % 4 == 0, 4 bytes otherwise\", \"z_chunk\": 16, "
         "\"reduction\": \"fp32 per lane, fp64 per wave, workgroup and list; no atomics\"}";
}

}  // namespace lp

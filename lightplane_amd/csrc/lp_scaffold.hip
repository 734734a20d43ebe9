// lp_scaffold.hip -- occupancy scaffold of a grid-list: the decoder's opacity on a regular lattice, thresholded and dilated, without a
// point, ray or encoding tensor and without float temporaries.
//
// Lattice kernel: one lane = one lattice point (b, z, y, x) of the [B, D, H, W] scaffold, one wave = one workgroup = 64 consecutive
// points.  The lane forms its own coordinates -- c(i, n) = fp32(torch.linspace(0, 1, n)[i] * 2 - 1), torch's two-sided formula (lin01,
// lp_device.h) --, gathers the grid-list exactly as the Renderer does (grid_corners<false>: the same corner rows and weights, the same
// summation order as sample_list) and evaluates trunk -> ReLU -> opacity MLP (two-grid mode: ReLU(features) -> opacity MLP) with
// runtime layer loops; opacity = gain * softplus(raw).  The colour MLP is never read.
//   activations: two LDS tiles [maxw][64], element i of lane l at (i * 64 + l): every lane reads and writes ITS column only, so there
//                is no barrier anywhere and a wave instruction touches 64 consecutive banks (conflict-free).  No private array, no
//                scratch: a runtime-indexed per-lane array would live in scratch memory.
//   weights:     wave-uniform addresses (kernel argument + uniform loop counters): scalar loads through the constant cache, one
//                s_load_dwordx8 per eight FMAs, for a decoder of any size -- nothing is staged, so nothing has to fit.
//   arithmetic:  plain fp32 FMA chains b + x[0] w[0] + x[1] w[1] + ... in ascending order (the shape-generic Renderer's).
// The result leaves as the raw opacity lattice, as 0 / 1 floats (opacity > threshold) or as occupancy bytes for the dilation.
//
// Dilation: max_pool3d(k = 2 r + 1, stride 1, padding r) followed by `> t` is the binary OR-dilation of `opacity > t` (the pad value
// -inf never wins and max commutes with the monotone map v -> v > t), and a box dilation is separable.  Three byte passes, along W, H
// and D, ping-pong between ONE byte per point of caller workspace and the first quarter of the output tensor; the last pass reads the
// workspace and writes the 0 / 1 floats.  No atomics, no host synchronisation: graph-capturable.
#include "lp_column_mlp.h"
#include "lp_host.h"

namespace lp {

constexpr int SC_DIL_THREADS = 256;

enum { SC_RAW = 0, SC_OCC_FLOAT = 1, SC_OCC_BYTE = 2 };

struct ScArgs {
  LpScaffoldArgs a;  // normalised: every grid carries its base pointer
  void* out;         // [B, D, H, W] floats (SC_RAW, SC_OCC_FLOAT) or bytes (SC_OCC_BYTE)
  int64_t n_points;
  int32_t maxw;      // rows of one activation tile
};

// (no second argument: the kernel takes 3x-4x fewer registers than the 128 that would cap a SIMD's eight waves; the LDS tiles bound
// the occupancy -- DESIGN.md 4.11)
template <int MODE>
__global__ void __launch_bounds__(SC_WAVE) scaffold_lattice(const ScArgs s) {
  extern __shared__ __attribute__((aligned(16))) float lds[];  // two activation tiles [maxw][64]
  const LpScaffoldArgs& a = s.a;
  const int lane = threadIdx.x;
  const int64_t p = (int64_t)blockIdx.x * SC_WAVE + lane;
  const bool valid = p < s.n_points;
  const int64_t q = valid ? p : s.n_points - 1;  // (a lane past the end recomputes the last point and stores nothing)
  const int W = a.shape.W, H = a.shape.H, D = a.shape.D;
  const LatticePoint at = lattice_point<int64_t>(q, W, H, D);
  const int ix = at.x, iy = at.y, iz = at.z, b = at.b;
  const float x = lin01(ix, W) * 2.0f - 1.0f;
  const float y = lin01(iy, H) * 2.0f - 1.0f;
  const float z = lin01(iz, D) * 2.0f - 1.0f;

  float* cur = lds + lane;
  float* nxt = lds + s.maxw * SC_WAVE + lane;
  const int C = a.grid.channels;
  sc_gather(a.grid, b, x, y, z, a.mask_out_of_bounds != 0, cur);
  if (a.trunk.n_layers == 0) {  // two-grid mode: the opacity head reads ReLU(features)
    for (int c = 0; c < C; ++c) cur[c * SC_WAVE] = fmaxf(cur[c * SC_WAVE], 0.0f);
  }
  for (int l = 0; l < a.trunk.n_layers; ++l) {
    sc_dense(mlp_w(a.mlp_params, a.trunk, l), mlp_b(a.mlp_params, a.trunk, l), a.trunk.dims[l], a.trunk.dims[l + 1],
             a.trunk.dims[l + 1], cur, nxt, true);
    float* t = cur;
    cur = nxt;
    nxt = t;
  }
  for (int l = 0; l < a.opacity.n_layers; ++l) {
    const bool last = l == a.opacity.n_layers - 1;
    sc_dense(mlp_w(a.mlp_params, a.opacity, l), mlp_b(a.mlp_params, a.opacity, l), a.opacity.dims[l], a.opacity.dims[l + 1],
             last ? 1 : a.opacity.dims[l + 1], cur, nxt, !last);
    float* t = cur;
    cur = nxt;
    nxt = t;
  }
  const float opacity = a.gain * softplus_f(cur[0]);
  if (!valid) return;
  if (MODE == SC_RAW) static_cast<float*>(s.out)[p] = opacity;
  else if (MODE == SC_OCC_FLOAT) static_cast<float*>(s.out)[p] = opacity > a.threshold ? 1.0f : 0.0f;
  else static_cast<uint8_t*>(s.out)[p] = opacity > a.threshold ? 1 : 0;
}

// One pass of the separable OR-dilation along an axis of extent n whose neighbours lie `stride` points apart:
// out[p] = OR of in[p + (j - i) * stride] over the j in [i - r, i + r] that are inside [0, n), i = the point's index on that axis.
// r <= n (the host clamps it: a larger window covers the whole axis all the same).
template <bool TO_FLOAT>
__global__ void __launch_bounds__(SC_DIL_THREADS) scaffold_dilate(const uint8_t* __restrict__ in, void* __restrict__ out, int64_t n_points,
                                                                  int32_t n, int64_t stride, int32_t r) {
  const int64_t p = (int64_t)blockIdx.x * SC_DIL_THREADS + threadIdx.x;
  if (p >= n_points) return;
  const int32_t i = (int32_t)((p / stride) % n);
  const int32_t lo = max(i - r, 0), hi = min(i + r, n - 1);
  const uint8_t* src = in + (p - (int64_t)(i - lo) * stride);
  unsigned v = 0;
  for (int32_t j = lo; j <= hi; ++j, src += stride) v |= *src;
  if (TO_FLOAT) static_cast<float*>(out)[p] = v ? 1.0f : 0.0f;
  else static_cast<uint8_t*>(out)[p] = v ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------

static int64_t scaffold_points(const LpGrid& s) { return (int64_t)s.B * s.D * s.H * s.W; }

// one byte per lattice point when there is a dilation to do, nothing otherwise
int64_t scaffold_workspace_bytes(const LpGrid& shape, int dilate) { return dilate > 0 ? scaffold_points(shape) : 0; }

// `a` normalised and checked by lp_api.hip.  occupancy == false: out = the raw opacity lattice (workspace unused).
// occupancy == true: out = dilate(opacity > threshold) as 0 / 1 floats, through `workspace` when a.dilate > 0.
int scaffold_launch(const LpScaffoldArgs& a, float* out, void* workspace, bool occupancy, hipStream_t stream) {
  ScArgs s;
  s.a = a;
  s.n_points = scaffold_points(a.shape);
  int maxw = a.grid.channels;
  const LpMlp* ms[2] = {&a.trunk, &a.opacity};
  for (const LpMlp* m : ms)
    for (int l = 0; l <= m->n_layers && m->n_layers > 0; ++l) maxw = m->dims[l] > maxw ? m->dims[l] : maxw;
  s.maxw = maxw;
  const size_t lds = (size_t)2 * maxw * SC_WAVE * sizeof(float);  // <= 64 KB (LP_MAX_WIDTH 128): within the default limit
  unsigned blocks;
  if (int rc = launch_blocks("lp_scaffold", s.n_points, SC_WAVE, blocks)) return rc;
  const dim3 gr(blocks), bl(SC_WAVE);
  if (!occupancy) {
    s.out = out;
    hipLaunchKernelGGL((scaffold_lattice<SC_RAW>), gr, bl, lds, stream, s);
    return check_launch("scaffold_lattice");
  }
  if (a.dilate <= 0) {
    s.out = out;
    hipLaunchKernelGGL((scaffold_lattice<SC_OCC_FLOAT>), gr, bl, lds, stream, s);
    return check_launch("scaffold_lattice");
  }
  uint8_t* const ws = static_cast<uint8_t*>(workspace);
  uint8_t* const ob = reinterpret_cast<uint8_t*>(out);  // the first quarter of the result as the second byte buffer
  s.out = ws;
  hipLaunchKernelGGL((scaffold_lattice<SC_OCC_BYTE>), gr, bl, lds, stream, s);
  int rc = check_launch("scaffold_lattice");
  if (rc) return rc;
  unsigned dblocks;
  if ((rc = launch_blocks("lp_scaffold", s.n_points, SC_DIL_THREADS, dblocks))) return rc;
  const dim3 dgr(dblocks), dbl(SC_DIL_THREADS);
  const int W = a.shape.W, H = a.shape.H, D = a.shape.D;
  hipLaunchKernelGGL((scaffold_dilate<false>), dgr, dbl, 0, stream, ws, (void*)ob, s.n_points, W, (int64_t)1, a.dilate < W ? a.dilate : W);
  if ((rc = check_launch("scaffold_dilate (W)"))) return rc;
  hipLaunchKernelGGL((scaffold_dilate<false>), dgr, dbl, 0, stream, ob, (void*)ws, s.n_points, H, (int64_t)W, a.dilate < H ? a.dilate : H);
  if ((rc = check_launch("scaffold_dilate (H)"))) return rc;
  // (the float pass reads the workspace, never the tensor it overwrites)
  hipLaunchKernelGGL((scaffold_dilate<true>), dgr, dbl, 0, stream, ws, (void*)out, s.n_points, D, (int64_t)H * W, a.dilate < D ? a.dilate : D);
  return check_launch("scaffold_dilate (D)");
}

const char* build_info_scaffold() {
  return "{\"lattice\": \"one lane per point, one wave per workgroup; fp32 FMA; activations in two LDS tiles [width][64], weights "
         "through wave-uniform scalar loads; runtime layer loops\", \"dilation\": \"separable OR of bytes (W, H, D), one byte per point of "
         "workspace ping-ponging with the result; no atomics\"}";
}

}  // namespace lp

// lp_column_mlp.h -- the decoder for one lane = one point with the activations in LDS column tiles [width][64]: the grid-list gather
// and the dense layer of the lattice kernel (lp_scaffold.hip) and of the point-evaluation forward (lp_points.hip).  Element i of lane l
// sits at (i * 64 + l): every lane reads and writes ITS column only, so there is no barrier and a wave instruction touches 64
// consecutive banks; weights come through wave-uniform scalar loads; plain fp32 FMA chains in ascending order; no private array.
#pragma once
#include "lp_generic_mlp.h"

namespace lp {

constexpr int SC_WAVE = 64;       // lanes of a lattice workgroup = row stride of the activation tiles

// Sum of the tri- / bi-linear samples of every grid of the list at (x, y, z) into the lane's LDS column out[c * 64], c < C: per channel
// the chain 0 + w0 v0 + w1 v1 + ... over grids and corners in list order, as sample_list() forms it.  A corner outside its grid
// contributes w = 0 times v = 0 (sample_list skips it: the same sum); its load goes to row 0 of the grid's tensor, which exists.
LP_DEV void sc_gather(const LpGridList& gl, int b, float x, float y, float z, bool mask_oob, float* out) {
  const int C = gl.channels;
  const bool live = !(mask_oob && !point_in_bounds(x, y, z));
  for (int g = 0; g < gl.n_grids; ++g) {
    const LpGrid& gd = gl.grids[g];
    const Corners cs = grid_corners<false>(gd, b, x, y, z);
    const int nk = (gd.D > 1 && gd.H > 1 && gd.W > 1) ? 8 : 4;  // wave-uniform: a property of the grid
    const float* rows[8];
    float w[8];
    bool ok[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      ok[k] = live && k < nk && cs.row[k] >= 0;
      rows[k] = gd.data + (ok[k] ? cs.row[k] : (int64_t)0) * C;
      w[k] = ok[k] ? cs.w[k] : 0.0f;
    }
    if ((C & 3) == 0) {
      for (int c = 0; c < C; c += 4) {
        float acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = g == 0 ? 0.0f : out[(c + j) * SC_WAVE];
        float4 v[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = *reinterpret_cast<const float4*>(rows[k] + c);
        if (nk == 8) {
#pragma unroll
          for (int k = 4; k < 8; ++k) v[k] = *reinterpret_cast<const float4*>(rows[k] + c);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          if (k < 4 || nk == 8) {
            acc[0] = fmaf(w[k], ok[k] ? v[k].x : 0.0f, acc[0]);
            acc[1] = fmaf(w[k], ok[k] ? v[k].y : 0.0f, acc[1]);
            acc[2] = fmaf(w[k], ok[k] ? v[k].z : 0.0f, acc[2]);
            acc[3] = fmaf(w[k], ok[k] ? v[k].w : 0.0f, acc[3]);
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) out[(c + j) * SC_WAVE] = acc[j];
      }
    } else {
      for (int c = 0; c < C; ++c) {
        float acc = g == 0 ? 0.0f : out[c * SC_WAVE];
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = (k < 4 || nk == 8) ? rows[k][c] : 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (k < 4 || nk == 8) acc = fmaf(w[k], ok[k] ? v[k] : 0.0f, acc);
        out[c * SC_WAVE] = acc;
      }
    }
  }
}

// y[o] = b[o] + sum_i x[i] * Wm[i * ldw + o], o < n_out, optionally through a ReLU.  x, y: LDS columns of the lane (stride 64), x != y.
// Wm, bias and every index into them are wave-uniform: scalar loads.  Blocks of eight outputs; the last, partial block (the opacity
// head's single output) re-reads its last column in the spare slots and does not store them.
// WP: const float*, or sc_const_ptr -- the same address in the constant address space, for a kernel that stores to global memory
// before it reads the weights again (a loop over chunks: lp_render_samples.hip).  The compiler issues scalar loads only for memory it
// knows the kernel does not write; behind a store it cannot tell, and the weights come through per-lane vector loads instead.
typedef const __attribute__((address_space(4))) float* sc_const_ptr;
LP_DEV sc_const_ptr sc_const(const float* p) { return (sc_const_ptr)p; }  // (p: global memory this kernel never writes)

template <typename WP>
LP_DEV void sc_dense(WP __restrict__ Wm, WP __restrict__ bias, int d_in, int ldw, int n_out, const float* x, float* y, bool relu) {
  int o0 = 0;
  for (; o0 + 8 <= n_out; o0 += 8) {
    float acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = bias[o0 + k];
    WP w = Wm + o0;
#pragma unroll 4
    for (int i = 0; i < d_in; ++i) {
      const float xi = x[i * SC_WAVE];
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] = fmaf(xi, w[k], acc[k]);
      w += ldw;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) y[(o0 + k) * SC_WAVE] = relu ? fmaxf(acc[k], 0.0f) : acc[k];
  }
  if (o0 < n_out) {
    const int rem = n_out - o0;
    int kk[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) kk[k] = k < rem ? k : rem - 1;
    float acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = bias[o0 + kk[k]];
    WP w = Wm + o0;
#pragma unroll 4
    for (int i = 0; i < d_in; ++i) {
      const float xi = x[i * SC_WAVE];
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] = fmaf(xi, w[kk[k]], acc[k]);
      w += ldw;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k < rem) y[(o0 + k) * SC_WAVE] = relu ? fmaxf(acc[k], 0.0f) : acc[k];
  }
}

}  // namespace lp

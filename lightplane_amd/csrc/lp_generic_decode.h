// lp_generic_decode.h -- the decoder of one point for one lane with private activation arrays: the activation plan, the argument
// block and the recompute shared by the shape-generic Renderer kernels (lp_renderer_generic.hip) and the point-evaluation backward
// (lp_points.hip), which is the Renderer backward without the march and the compositing.
#pragma once
#include "lp_generic_mlp.h"
#include "lp_host.h"

namespace lp {

// Offsets (in floats) of every activation of one sample inside the private array.
struct GenPlan {
  int x0;                   // [C] summed grid sample (raw)
  int cx0;                  // [C] colour-grid sample (raw) or -1
  int trunk[LP_MAX_LAYERS]; // trunk layer outputs (post ReLU)
  int op_in;                // opacity head input (post ReLU)
  int col_in;               // colour head input (+ encoding)
  int op[LP_MAX_LAYERS];    // opacity layer outputs (hidden: post ReLU, last: raw)
  int col[LP_MAX_LAYERS];   // colour layer outputs (hidden: post ReLU, last: raw, color_chn used)
  int total;
  int head_w;               // width of the head inputs
};

struct GenArgs {
  LpRendererArgs a;
  GenPlan p;
  int stage_ld;        // LDS staging row stride (floats), bwd only
  int lds_param_accum; // 1: accumulate weight grads in LDS, flush once per block
  // test hook (lp_renderer_backward_relu_dump, DUMP twin only): [ray][sample][dump_words] words -- dump_wps words per ReLU site in the
  // reference's evaluation order, then the visited flag
  uint32_t* relu_dump;
  int dump_words, dump_wps;
};

// Full decoder of one sample.  Fills act[] per plan; returns the raw opacity (pre noise).
// The raw colours are left in act[p.col[nC-1] .. +color_chn).
// Layers of 24 and more outputs run for the whole wave on the fp32 matrix cores (dense_wave, lp_generic_mlp.h; Xs: the wave's LDS tile
// [64][ga.stage_ld]); the narrow ones (the heads' output layers) stay per lane.  Wave-uniform control flow.
LP_DEV void dense_any(const float* W, const float* b, int d_in, int ldw, int n_out, const float* x, float* y, bool relu, float* Xs,
                      int ld, int lane) {
  if (dense_on_mfma(d_in, n_out))
    dense_wave(W, b, d_in, ldw, n_out, x, y, relu, Xs, ld, lane);
  else
    dense(W, b, d_in, ldw, n_out, x, y, relu);
}

LP_DEV float decode(const GenArgs& ga, const Ray& ray, float x, float y, float z,
                    const float* enc, float* act, float* Xs, int lane) {
  const LpRendererArgs& a = ga.a;
  const GenPlan& p = ga.p;
  const bool mask = a.march.mask_out_of_bounds != 0;
  const bool two_grids = a.color_grid.n_grids > 0;
  const int C = a.grid.channels;
  sample_list(a.grid, ray.b, x, y, z, mask, act + p.x0);
  if (two_grids) {
    sample_list(a.color_grid, ray.b, x, y, z, mask, act + p.cx0);
    for (int c = 0; c < C; ++c) {
      act[p.op_in + c] = fmaxf(act[p.x0 + c], 0.0f);
      act[p.col_in + c] = fmaxf(act[p.cx0 + c], 0.0f) + enc[c];
    }
  } else {
    const float* cur = act + p.x0;
    int w = C;
    for (int l = 0; l < a.trunk.n_layers; ++l) {
      dense_any(mlp_w(a.mlp_params, a.trunk, l), mlp_b(a.mlp_params, a.trunk, l), a.trunk.dims[l],
                a.trunk.dims[l + 1], a.trunk.dims[l + 1], cur, act + p.trunk[l], true, Xs, ga.stage_ld, lane);
      cur = act + p.trunk[l];
      w = a.trunk.dims[l + 1];
    }
    if (a.trunk.n_layers == 0) {
      for (int c = 0; c < C; ++c) act[p.op_in + c] = fmaxf(act[p.x0 + c], 0.0f);
      cur = act + p.op_in;
    }
    {
      int c = 0;
      for (; c + 8 <= w; c += 8) {  // (eight reads of each private array in flight)
        float u8[8], e8[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          u8[q] = cur[c + q];
          e8[q] = enc[c + q];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) act[p.col_in + c + q] = u8[q] + e8[q];
      }
      for (; c < w; ++c) act[p.col_in + c] = cur[c] + enc[c];
    }
  }
  // opacity head
  {
    const float* cur = act + p.op_in;
    const LpMlp& m = a.opacity;
    for (int l = 0; l < m.n_layers; ++l) {
      const bool last = (l == m.n_layers - 1);
      dense_any(mlp_w(a.mlp_params, m, l), mlp_b(a.mlp_params, m, l), m.dims[l], m.dims[l + 1],
                last ? 1 : m.dims[l + 1], cur, act + p.op[l], !last, Xs, ga.stage_ld, lane);
      cur = act + p.op[l];
    }
  }
  // colour head
  {
    const float* cur = act + p.col_in;
    const LpMlp& m = a.color;
    for (int l = 0; l < m.n_layers; ++l) {
      const bool last = (l == m.n_layers - 1);
      dense_any(mlp_w(a.mlp_params, m, l), mlp_b(a.mlp_params, m, l), m.dims[l], m.dims[l + 1],
                last ? a.color_chn : m.dims[l + 1], cur, act + p.col[l], !last, Xs, ga.stage_ld, lane);
      cur = act + p.col[l];
    }
  }
  return act[p.op[a.opacity.n_layers - 1]];
}

// The same without the colour branch (the point-evaluation backward without a colour gradient): grid-list -> trunk -> opacity head.
// The colour grid-list is not sampled and the colour head not evaluated; act[] holds nothing for them.
LP_DEV float decode_opacity(const GenArgs& ga, const Ray& ray, float x, float y, float z, float* act, float* Xs, int lane) {
  const LpRendererArgs& a = ga.a;
  const GenPlan& p = ga.p;
  const int C = a.grid.channels;
  sample_list(a.grid, ray.b, x, y, z, a.march.mask_out_of_bounds != 0, act + p.x0);
  const float* cur = act + p.x0;
  for (int l = 0; l < a.trunk.n_layers; ++l) {
    dense_any(mlp_w(a.mlp_params, a.trunk, l), mlp_b(a.mlp_params, a.trunk, l), a.trunk.dims[l], a.trunk.dims[l + 1],
              a.trunk.dims[l + 1], cur, act + p.trunk[l], true, Xs, ga.stage_ld, lane);
    cur = act + p.trunk[l];
  }
  if (a.trunk.n_layers == 0) {  // (also the two-grid decoder: make_plan gives it an op_in slot of its own)
    for (int c = 0; c < C; ++c) act[p.op_in + c] = fmaxf(act[p.x0 + c], 0.0f);
  }
  cur = act + p.op_in;
  const LpMlp& m = a.opacity;
  for (int l = 0; l < m.n_layers; ++l) {
    const bool last = (l == m.n_layers - 1);
    dense_any(mlp_w(a.mlp_params, m, l), mlp_b(a.mlp_params, m, l), m.dims[l], m.dims[l + 1], last ? 1 : m.dims[l + 1], cur,
              act + p.op[l], !last, Xs, ga.stage_ld, lane);
    cur = act + p.op[l];
  }
  return act[p.op[m.n_layers - 1]];
}

inline int make_plan(const LpRendererArgs& a, GenPlan& p) {
  int pos = 0;
  const int C = a.grid.channels;
  const bool two = a.color_grid.n_grids > 0;
  p.x0 = pos; pos += C;
  p.cx0 = -1;
  if (two) { p.cx0 = pos; pos += C; }
  int w = C;
  for (int l = 0; l < a.trunk.n_layers; ++l) { p.trunk[l] = pos; pos += a.trunk.dims[l + 1]; w = a.trunk.dims[l + 1]; }
  if (!two && a.trunk.n_layers > 0) {
    p.op_in = p.trunk[a.trunk.n_layers - 1];
  } else {
    p.op_in = pos; pos += C; w = C;
  }
  p.head_w = w;
  p.col_in = pos; pos += w;
  for (int l = 0; l < a.opacity.n_layers; ++l) { p.op[l] = pos; pos += a.opacity.dims[l + 1]; }
  for (int l = 0; l < a.color.n_layers; ++l) { p.col[l] = pos; pos += a.color.dims[l + 1]; }
  p.total = pos;
  return pos;
}

// row stride (floats) of the waves' LDS staging tiles: the widest layer input / output + 1 (odd for the usual even widths:
// conflict-free rows)
inline int generic_stage_ld(const LpRendererArgs& a) {
  int maxw = a.grid.channels;
  const LpMlp* ms[3] = {&a.trunk, &a.opacity, &a.color};
  for (const LpMlp* m : ms)
    for (int l = 0; l <= m->n_layers && m->n_layers > 0; ++l) maxw = m->dims[l] > maxw ? m->dims[l] : maxw;
  return maxw + 1;
}

}  // namespace lp

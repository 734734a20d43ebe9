// lp_render_samples.hip -- rendering at caller-given sample depths: decoder and compositing in one launch, forward and backward
// (C ABI lp_render_samples_forward / lp_render_samples_backward of include/lightplane_hip_render_samples.h).
//
// Both kernels: one wavefront = one workgroup works on one ray at a time, lanes = samples, chunks of 64 samples with carries.  The depth
// rows are read coalesced, the point depth * direction + origin is formed in registers (sample_point: the arithmetic of ray_samples and
// importance_samples, whose points the chain reads back from memory), and nothing of size [n_rays, n_samples] is written but the
// weights the caller asks for.
//
// Forward, render_samples_fwd: per chunk the lane decodes its sample with the body of points_fwd (lp_points.hip: activations in LDS
// column tiles [maxw][64], sc_gather / sc_dense, no scratch; the weights are read through the constant address space, so that they
// stay scalar loads behind the stores of the chunk before), the wave scans od = opacity * delta as composite_fwd does
// (lp_composite.hip) and stores the -log T the chunk starts from to chunk_nlt[ray][chunk].  The colour sums: every lane leaves w *
// colour in its LDS column, then lane c adds channel c over the chunk's 64 samples in ascending order -- a fixed order, so the result
// is bit-reproducible.  A lane past S works on sample 0 and contributes nothing.
//
// Backward, render_samples_bwd: a workgroup takes a run of consecutive rays (as points_bwd takes tiles: the weight gradients live in
// LDS accumulators that are flushed once per workgroup) and walks a ray's chunks far -> near.  The lane recomputes its sample with
// decode() (lp_generic_decode.h), T comes from chunk_nlt plus the scan inside the chunk, the suffix sums from wave_rscan with a carry
// (composite_bwd), and the decoder's upstream gradients
//   d raw = d_od * delta * gain * occ * softplus'(raw),   d craw[c] = w * g_feat[c] * occ * sigmoid'(craw[c])
// are formed in registers and handed to the body of points_bwd: mlp_backward, splat_list_wave.  The encoding gradient is accumulated
// per lane over the ray's chunks, summed over the lanes in a fixed order through the staging tile and STORED: no atomics for it.
#include "lp_column_mlp.h"
#include "lp_generic_decode.h"
#include "lp_point_grad.h"
#include "lp_wave.h"

namespace lp {

namespace {

struct RsFwdArgs {
  LpRenderSamplesArgs a;  // normalised: every grid carries its base pointer
  int32_t maxw;           // rows of one activation tile
  int32_t n_chunks;
};

LP_DEV Ray sample_ray(const float* origins, const float* directions, int64_t r, int b) {
  Ray q;
  load_ray_line(origins, directions, r, q);
  q.near_t = q.far_t = 0.0f;
  q.b = b;
  return q;
}

// sum + p[0] + p[stride] + ... + p[63 * stride] in that order (LDS), the reads issued sixteen at a time: one dependent read per add
// is 64 LDS latencies per call
LP_DEV float column_sum(const float* p, int stride, float sum) {
  for (int j0 = 0; j0 < 64; j0 += 16) {
    float v[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] = p[(j0 + q) * stride];
#pragma unroll
    for (int q = 0; q < 16; ++q) sum += v[q];
  }
  return sum;
}

// dynamic LDS: three activation tiles [maxw][64]
__global__ void __launch_bounds__(SC_WAVE) render_samples_fwd(const RsFwdArgs s) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const LpRenderSamplesArgs& a = s.a;
  const int lane = threadIdx.x;
  const int64_t r = blockIdx.x;
  const int S = a.n_samples;
  const int64_t base = r * S;
  const Ray ray = sample_ray(a.origins, a.directions, r, clamp_batch(a.grid_idx[r], a.grid.grids[0].B));
  const bool mask = a.mask_out_of_bounds != 0;
  const bool contract = a.contract_coords != 0;
  const int C = a.grid.channels;
  const int Cc = a.color_chn;
  const float* e = a.encoding + r * a.encoding_dim;
  float carry = 0.0f, len = 0.0f;
  float facc[2] = {0.0f, 0.0f};  // lane c: channels c and 64 + c of the feature sums

  for (int k = 0; k < s.n_chunks; ++k) {
    const int64_t sm = (int64_t)k * 64 + lane;  // (64-bit: the last chunk of a ray of nearly 2^31 samples ends beyond it)
    const bool in = sm < S;
    const int64_t at = base + (in ? sm : 0);
    const float dp = a.depths[at];
    const float dl = a.deltas[at];
    float x, y, z;
    sample_point(ray, dp, contract, x, y, z);
    float occ = 1.0f;
    if (a.scaffold) occ = scaffold_lookup(a.scaffold, a.scaffold_shape, ray.b, x, y, z);

    // ---- the decoder: the body of points_fwd<false> ----
    float* cur = lds + lane;
    float* nxt = lds + s.maxw * SC_WAVE + lane;
    sc_gather(a.grid, ray.b, x, y, z, mask, cur);
    if (a.trunk.n_layers == 0) {  // the heads read ReLU(features)
      for (int c = 0; c < C; ++c) cur[c * SC_WAVE] = fmaxf(cur[c * SC_WAVE], 0.0f);
    }
    int hw = C;  // width of the heads' input
    for (int l = 0; l < a.trunk.n_layers; ++l) {
      sc_dense(sc_const(mlp_w(a.mlp_params, a.trunk, l)), sc_const(mlp_b(a.mlp_params, a.trunk, l)), a.trunk.dims[l], a.trunk.dims[l + 1],
               a.trunk.dims[l + 1], cur, nxt, true);
      hw = a.trunk.dims[l + 1];
      float* t = cur;
      cur = nxt;
      nxt = t;
    }
    float* cin = lds + 2 * s.maxw * SC_WAVE + lane;  // the colour head's input (third tile)
    if (a.color_grid.n_grids > 0) {
      sc_gather(a.color_grid, ray.b, x, y, z, mask, cin);
      for (int c = 0; c < C; ++c) cin[c * SC_WAVE] = fmaxf(cin[c * SC_WAVE], 0.0f) + e[c];
    } else {
      for (int c = 0; c < hw; ++c) cin[c * SC_WAVE] = cur[c * SC_WAVE] + e[c];
    }
    for (int l = 0; l < a.opacity.n_layers; ++l) {
      const bool last = l == a.opacity.n_layers - 1;
      sc_dense(sc_const(mlp_w(a.mlp_params, a.opacity, l)), sc_const(mlp_b(a.mlp_params, a.opacity, l)), a.opacity.dims[l], a.opacity.dims[l + 1],
               last ? 1 : a.opacity.dims[l + 1], cur, nxt, !last);
      float* t = cur;
      cur = nxt;
      nxt = t;
    }
    const float opacity = a.gain * softplus_f(cur[0]) * occ;
    cur = cin;  // (both other tiles are free now)
    for (int l = 0; l < a.color.n_layers; ++l) {
      const bool last = l == a.color.n_layers - 1;
      sc_dense(sc_const(mlp_w(a.mlp_params, a.color, l)), sc_const(mlp_b(a.mlp_params, a.color, l)), a.color.dims[l], a.color.dims[l + 1],
               last ? Cc : a.color.dims[l + 1], cur, nxt, !last);
      float* t = cur;
      cur = nxt;
      nxt = t;
    }

    // ---- compositing: the scan of composite_fwd ----
    const float od = in ? opacity * dl : 0.0f;
    const float incl = wave_scan(od, lane);
    const float up = __shfl_up(incl, 1, 64);
    const float nlt = carry + (lane > 0 ? up : 0.0f);  // -log T in front of the sample
    const float w = in ? expf(-nlt) * (-expm1f(-od)) : 0.0f;
    len += w * dp;
    if (a.weights && in) a.weights[at] = w;
    if (a.chunk_nlt && lane == 0) a.chunk_nlt[r * s.n_chunks + k] = carry;
    carry += __shfl(incl, 63, 64);
    // w * colour into the lane's column of the tile the colour head ended in, then lanes = channels over the samples in ascending order
    for (int c = 0; c < Cc; ++c) cur[c * SC_WAVE] = in ? w * (sigmoid_f(cur[c * SC_WAVE]) * occ) : 0.0f;
    __syncthreads();
    const float* tile = cur - lane;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = lane + 64 * h;
      if (c < Cc) facc[h] = column_sum(tile + c * SC_WAVE, 1, facc[h]);
    }
    __syncthreads();
  }
  len = wave_sum(len);
  if (lane == 0) {
    if (a.ray_length) a.ray_length[r] = len;
    if (a.neg_log_t) a.neg_log_t[r] = carry;
  }
  if (a.feature) {
    if (lane < Cc) a.feature[r * Cc + lane] = facc[0];
    if (lane + 64 < Cc) a.feature[r * Cc + lane + 64] = facc[1];
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------------------------------------

struct RsBwdArgs {
  GenArgs ga;  // the decoder, the grids and the result gradients in the generic Renderer's argument block
  const float *origins, *directions, *depths, *deltas, *chunk_nlt;
  const float *g_len, *g_nlt, *g_feat, *g_w;
  float* grad_encoding;    // [n_rays, enc_dim], written (ga.a.grad_encoding stays NULL: nothing is added atomically)
  int32_t S, n_chunks;
  int32_t rays_per_block;  // consecutive rays of one workgroup
  int32_t color;           // the colour head takes part (g_feat given)
  int32_t enc_dim;         // columns of grad_encoding (ga.a.rays.encoding_dim is 0 without the colour head)
};

// dynamic LDS: Xs[64][ld] | Ys[64][ld] | (LDS_ACC) the weight-gradient accumulators [n_mlp_params]
template <int ACT_CAP, bool LDS_ACC>
__global__ void __launch_bounds__(64) render_samples_bwd(const RsBwdArgs s) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const GenArgs& ga = s.ga;
  const LpRendererArgs& a = ga.a;
  const GenPlan& p = ga.p;
  const int lane = threadIdx.x;

  float* Xs = lds;
  float* Ys = lds + 64 * ga.stage_ld;
  float* gparams_lds = lds + 128 * ga.stage_ld;
  float* gparams = nullptr;
  if (a.grad_mlp_params) {
    if (LDS_ACC) {
      for (int64_t i = lane; i < a.n_mlp_params; i += 64) gparams_lds[i] = 0.0f;
      gparams = gparams_lds;
    } else {
      gparams = a.grad_mlp_params;
    }
  }
  __syncthreads();

  float act[ACT_CAP];
  float enc[LP_MAX_WIDTH], genc[LP_MAX_WIDTH];
  float dy[LP_MAX_WIDTH], dx[LP_MAX_WIDTH], dhead[LP_MAX_WIDTH];
  const int E = a.rays.encoding_dim;
  const int Cc = a.color_chn;
  const bool contract = a.march.contract_coords != 0;
  const bool mask = a.march.mask_out_of_bounds != 0;
  const bool two_grids = a.color_grid.n_grids > 0;
  const bool color = s.color != 0;  // wave-uniform
  const int C = a.grid.channels;
  const int hw = p.head_w;
  const int craw = color ? p.col[a.color.n_layers - 1] : 0;
  const int S = s.S;

  for (int t = 0; t < s.rays_per_block; ++t) {
    const int64_t r = (int64_t)blockIdx.x * s.rays_per_block + t;
    if (r >= a.rays.n_rays) break;  // wave-uniform
    const Ray ray = sample_ray(s.origins, s.directions, r, clamp_batch(a.rays.grid_idx[r], a.grid.grids[0].B));
    const int64_t base = r * S;
    const float gl = s.g_len ? s.g_len[r] : 0.0f;
    const float gn = s.g_nlt ? s.g_nlt[r] : 0.0f;
    const float* gf = color ? s.g_feat + r * Cc : nullptr;
    if (color)
      for (int c = 0; c < E; ++c) {
        enc[c] = a.rays.encoding[r * E + c];
        genc[c] = 0.0f;
      }
    float rev = 0.0f;  // sum of w v over the chunks behind

    for (int k = s.n_chunks - 1; k >= 0; --k) {
      const int64_t sm = (int64_t)k * 64 + lane;  // (64-bit: the last chunk of a ray of nearly 2^31 samples ends beyond it)
      const bool live = sm < S;
      const int64_t at = base + (live ? sm : 0);  // (a lane past the end recomputes sample 0 and contributes nothing)
      const float dp = s.depths[at];
      const float dl = s.deltas[at];
      float x, y, z;
      sample_point(ray, dp, contract, x, y, z);
      float occ = 1.0f;
      if (a.scaffold) occ = scaffold_lookup(a.scaffold, a.scaffold_shape, ray.b, x, y, z);
      const float raw = color ? decode(ga, ray, x, y, z, enc, act, Xs, lane) : decode_opacity(ga, ray, x, y, z, act, Xs, lane);

      // ---- compositing backward: the chunk step of composite_bwd ----
      const float o = a.gain * softplus_f(raw) * occ;
      const float od = live ? o * dl : 0.0f;
      const float c0 = s.chunk_nlt[r * s.n_chunks + k];
      const float incl = wave_scan(od, lane);
      const float up = __shfl_up(incl, 1, 64);
      const float t_next = expf(-(c0 + incl));  // T behind the sample
      const float w = live ? expf(-(c0 + (lane > 0 ? up : 0.0f))) * (-expm1f(-od)) : 0.0f;
      float dot = 0.0f;
      if (color)
        for (int c = 0; c < Cc; ++c) dot = fmaf(gf[c], sigmoid_f(act[craw + c]) * occ, dot);
      const float gw = (live && s.g_w) ? s.g_w[at] : 0.0f;
      const float v = gl * dp + dot + gw;
      const float rincl = wave_rscan(live ? w * v : 0.0f, lane);
      const float down = __shfl_down(rincl, 1, 64);
      const float behind = rev + (lane < 63 ? down : 0.0f);
      const float d_od = t_next * v - behind + gn;
      rev += __shfl(rincl, 0, 64);
      const float d_raw_op = live ? d_od * dl * a.gain * occ * d_softplus_f(raw) : 0.0f;

      // ---- the decoder backward: the body of points_bwd ----
      auto scatter = [&](const LpGridList& gl_, float* const* grad, const float* d) {
        if (splat_wave_ok(ga.stage_ld))
          splat_list_wave(gl_, grad, ray.b, x, y, z, mask, d, live, Xs, Ys, ga.stage_ld, lane);
        else if (live)
          splat_list(gl_, grad, ray.b, x, y, z, mask, d);
      };
      if (color) {
        for (int c = 0; c < Cc; ++c) {
          const float sg = sigmoid_f(act[craw + c]);
          dy[c] = live ? w * gf[c] * occ * sg * (1.0f - sg) : 0.0f;
        }
        mlp_backward<LDS_ACC>(a.mlp_params, ga.stage_ld, a.color, Cc, p.col_in, p.col, act, dy, dx, gparams, Xs, Ys, lane, live);
        for (int c = 0; c < hw; ++c) dhead[c] = dx[c];
        if (s.grad_encoding)
          for (int c = 0; c < E; ++c) genc[c] += live ? dx[c] : 0.0f;
      } else {
        for (int c = 0; c < hw; ++c) dhead[c] = 0.0f;
      }
      dy[0] = d_raw_op;
      mlp_backward<LDS_ACC>(a.mlp_params, ga.stage_ld, a.opacity, 1, p.op_in, p.op, act, dy, dx, gparams, Xs, Ys, lane, live);
      if (two_grids) {
        // opacity input = relu(x0), colour input = relu(cx0) + enc
        for (int c = 0; c < C; ++c) dx[c] = (act[p.x0 + c] > 0.0f) ? dx[c] : 0.0f;
        if (a.grad_grid_list[0]) scatter(a.grid, a.grad_grid_list, dx);
        if (color) {
          for (int c = 0; c < C; ++c) dhead[c] = (act[p.cx0 + c] > 0.0f) ? dhead[c] : 0.0f;
          if (a.grad_color_grid_list[0]) scatter(a.color_grid, a.grad_color_grid_list, dhead);
        }
      } else {
        // trunk output gradient = colour-input grad + opacity-input grad, through the ReLU
        for (int c = 0; c < hw; ++c) {
          const float g = dhead[c] + dx[c];
          dy[c] = (act[p.op_in + c] > 0.0f) ? g : 0.0f;
        }
        if (a.trunk.n_layers > 0) {
          const LpMlp& m = a.trunk;
          mlp_backward<LDS_ACC>(a.mlp_params, ga.stage_ld, m, m.dims[m.n_layers], p.x0, p.trunk, act, dy, dx, gparams, Xs, Ys, lane, live);
        } else {
          for (int c = 0; c < C; ++c) dx[c] = dy[c];
        }
        if (a.grad_grid_list[0]) scatter(a.grid, a.grad_grid_list, dx);
      }
    }

    // the ray's encoding gradient: the lanes' sums through the staging tile, lanes = channels over its 64 rows in ascending order
    if (s.grad_encoding) {
      float* out = s.grad_encoding + r * s.enc_dim;
      if (color) {
        stage(Xs, ga.stage_ld, lane, genc, E, false);
        __syncthreads();
        for (int c = lane; c < E; c += 64) out[c] = column_sum(Xs + c, ga.stage_ld, 0.0f);
        __syncthreads();
      } else {
        for (int c = lane; c < s.enc_dim; c += 64) out[c] = 0.0f;
      }
    }
  }
  if (LDS_ACC && a.grad_mlp_params) {
    __syncthreads();
    for (int64_t i = lane; i < a.n_mlp_params; i += 64) {
      const float v = gparams_lds[i];
      if (v != 0.0f) atomic_add_f32(a.grad_mlp_params + i, v);
    }
  }
}

constexpr int64_t RS_BWD_BLOCKS = 2048;  // workgroups a large backward is cut into (as the point-evaluation backward)

int widest(const LpRenderSamplesArgs& a) {
  int maxw = a.grid.channels;
  const LpMlp* ms[3] = {&a.trunk, &a.opacity, &a.color};
  for (const LpMlp* m : ms)
    for (int l = 0; l <= m->n_layers && m->n_layers > 0; ++l) maxw = m->dims[l] > maxw ? m->dims[l] : maxw;
  return maxw;
}

// the generic Renderer's argument block of the decoder: grids, scaffold, MLPs and the atomically accumulated result gradients
void renderer_view(const LpRenderSamplesArgs& a, bool color, LpRendererArgs& ra) {
  ra = LpRendererArgs{};
  ra.rays.n_rays = a.n_rays;
  ra.rays.grid_idx = a.grid_idx;
  ra.rays.encoding = a.encoding;
  ra.rays.encoding_dim = color ? a.encoding_dim : 0;
  ra.grid = a.grid;
  ra.color_grid = a.color_grid;
  ra.scaffold = a.scaffold;
  ra.scaffold_shape = a.scaffold_shape;
  ra.march.num_samples = a.n_samples;
  ra.march.mask_out_of_bounds = a.mask_out_of_bounds;
  ra.march.contract_coords = a.contract_coords;
  ra.mlp_params = a.mlp_params;
  ra.n_mlp_params = a.n_mlp_params;
  ra.trunk = a.trunk;
  ra.opacity = a.opacity;
  ra.color = a.color;
  if (!color) ra.color.n_layers = 0;
  ra.color_chn = a.color_chn;
  ra.gain = a.gain;
  ra.grad_mlp_params = a.grad_mlp_params;
  for (int g = 0; g < LP_MAX_GRIDS; ++g) {
    ra.grad_grid_list[g] = a.grad_grid_list[g];
    ra.grad_color_grid_list[g] = color ? a.grad_color_grid_list[g] : nullptr;
  }
}

int forward_launch(const LpRenderSamplesArgs& a, hipStream_t stream) {
  RsFwdArgs s;
  s.a = a;
  s.maxw = widest(a);
  s.n_chunks = lp_render_samples_chunks(a.n_samples);
  const size_t lds = (size_t)3 * s.maxw * SC_WAVE * sizeof(float);  // <= 96 KB (LP_MAX_WIDTH 128)
  // (one workgroup per ray: lp_api.hip keeps n_rays * n_samples, hence n_rays, below 2^31)
  unsigned blocks;
  if (int rc = launch_blocks("lp_render_samples_forward", a.n_rays, 1, blocks)) return rc;
  const hipError_t e = hipFuncSetAttribute((const void*)render_samples_fwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return set_error((int)e, "hipFuncSetAttribute: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(render_samples_fwd, dim3(blocks), dim3(SC_WAVE), lds, stream, s);
  return check_launch("render_samples_fwd");
}

int backward_launch(const LpRenderSamplesArgs& a, hipStream_t stream) {
  if (!a.grad_ray_length && !a.grad_neg_log_t && !a.grad_feature && !a.grad_weights) return LP_OK;  // every result is zero
  RsBwdArgs s;
  const bool color = a.grad_feature != nullptr;
  renderer_view(a, color, s.ga.a);
  const LpRendererArgs& ra = s.ga.a;
  const int total = make_plan(ra, s.ga.p);
  if (total > 1024) return set_error(LP_EUNSUPPORTED, "lp_render_samples_backward: sum of layer widths %d exceeds 1024", total);
  s.ga.stage_ld = generic_stage_ld(ra);
  s.ga.relu_dump = nullptr;
  s.ga.dump_words = s.ga.dump_wps = 0;
  s.origins = a.origins, s.directions = a.directions, s.depths = a.depths, s.deltas = a.deltas, s.chunk_nlt = a.chunk_nlt;
  s.g_len = a.grad_ray_length, s.g_nlt = a.grad_neg_log_t, s.g_feat = a.grad_feature, s.g_w = a.grad_weights;
  s.grad_encoding = a.grad_encoding;
  s.S = a.n_samples;
  s.n_chunks = lp_render_samples_chunks(a.n_samples);
  s.color = color ? 1 : 0;
  s.enc_dim = a.encoding_dim;
  const size_t stage_bytes = (size_t)128 * s.ga.stage_ld * sizeof(float);
  const size_t param_bytes = (size_t)a.n_mlp_params * sizeof(float);
  const bool lds_acc = a.grad_mlp_params && (stage_bytes + param_bytes <= 96 * 1024);
  s.ga.lds_param_accum = lds_acc ? 1 : 0;
  const size_t lds = stage_bytes + (lds_acc ? param_bytes : 0);
  int64_t rpb;
  workgroup_count(a.n_rays, RS_BWD_BLOCKS, rpb);  // (n_rays < 2^31)
  s.rays_per_block = (int32_t)rpb;
  unsigned blocks;
  if (int rc = launch_blocks("lp_render_samples_backward", a.n_rays, rpb, blocks)) return rc;
#define LP_LAUNCH_RS_BWD(CAP, ACC)                                                                                                        \
  do {                                                                                                                                    \
    hipError_t e = hipFuncSetAttribute((const void*)render_samples_bwd<CAP, ACC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    if (e != hipSuccess) return set_error((int)e, "hipFuncSetAttribute: %s", hipGetErrorString(e));                                       \
    hipLaunchKernelGGL((render_samples_bwd<CAP, ACC>), dim3(blocks), dim3(64), lds, stream, s);                                           \
  } while (0)
  if (total <= 256) {
    if (lds_acc) LP_LAUNCH_RS_BWD(256, true); else LP_LAUNCH_RS_BWD(256, false);
  } else {
    if (lds_acc) LP_LAUNCH_RS_BWD(1024, true); else LP_LAUNCH_RS_BWD(1024, false);
  }
#undef LP_LAUNCH_RS_BWD
  return check_launch("render_samples_bwd");
}

}  // namespace

// `a` normalised and checked by lp_api.hip: n_rays > 0, n_samples >= 1, n_rays * n_samples < 2^31
int render_samples_launch(const LpRenderSamplesArgs& a, bool backward, hipStream_t stream) {
  return backward ? backward_launch(a, stream) : forward_launch(a, stream);
}

const char* build_info_render_samples() {
  return "{\"forward\": \"one wavefront per ray, lanes = samples in chunks of 64: the decoder of the points forward (LDS column tiles, fp32 "
         "FMA, no scratch) and the compositing scan in one launch; fixed-order sums\", \"backward\": \"one wavefront per ray, chunks far to "
         "near from the saved per-chunk -log T: the recompute and the decoder backward of the points backward; encoding gradient stored "
         "per ray, no atomics\"}";
}

}  // namespace lp

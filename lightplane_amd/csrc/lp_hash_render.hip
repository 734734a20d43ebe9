// lp_hash_render.hip -- a multiresolution hash-grid field rendered along rays at caller-given sample depths: encoding, decoder and
// compositing in one launch, forward and backward (C ABI lp_hash_render_forward / lp_hash_render_backward of
// include/lightplane_hip_hash_render.h, which holds the definition).  It is the product of lp_hash_points.hip (the field at points)
// and lp_render_samples.hip (decode + composite along a ray), and replaces the chain ray_samples -> hash_points -> composite without
// its [n_rays, n_samples] tensors: points, opacity, colour and their gradients never reach memory.
//
// Both kernels: one wavefront = one workgroup works on ONE RAY at a time, lanes = samples, chunks of 64 with the -log T carried
// between them -- not the point-major tiling of hash_points, where a ray boundary may fall inside a wave.  What that buys:
//   * the batch element b is wave-uniform (readfirstlane makes it so for the compiler): every level's table base hg_base(b, level)
//     and the ray's encoding row live in SGPRs, a lane carries only its entry offsets;
//   * consecutive lanes are consecutive depths of one ray, so on the coarse levels they share cells: the table gradient of the
//     backward merges whole stretches of the wave into one atomic per corner (hg_run_ray: no batch comparison per lane).
//
// Forward, hash_render_fwd<OPACITY_ONLY>: per chunk the lane forms its point in registers (sample_point: the arithmetic of
// ray_samples / importance_samples, whose points the chain reads back), computes mask and scaffold once, loops over the levels
// (hp_features, lp_hash_levels.h: level constants through a wave-uniform index, the 8 corner loads issued together, F dispatched by
// a wave-uniform switch) into rows l F .. of the first LDS column tile [maxw][64], and runs the decoder of hash_points_fwd with the
// weights read through the constant address space (sc_const: scalar loads that stay scalar behind the stores of the chunk before).
// Then the scan of composite_fwd and the colour fold of render_samples_fwd: w * colour left in the lane's column, lane c sums channel
// c in ascending order.  No private array and no atomics: every result is bit-reproducible (the compiler spills 67 - 83 scalars of
// the argument block, 20 bytes of scratch per lane: DESIGN.md 4.24).  A lane past S works on sample 0 and contributes nothing.  OPACITY_ONLY (feature == NULL): two tiles instead of three, the colour MLP and the encoding are never read.
//
// Backward, hash_render_bwd<ACT_CAP, LDS_ACC>: a workgroup takes a run of consecutive rays and walks each ray's chunks far -> near.
// The lane recomputes its features into act[x0 ..] and the decoder behind them (decode_gathered, lp_generic_decode.h), T comes from
// chunk_nlt plus the scan inside the chunk, the suffix sums from wave_rscan with a carry, and
//   d raw = d_od * delta * gain * occ * softplus'(raw),   d craw[c] = w * g_feat[c] * occ * sigmoid'(craw[c])
// go through mlp_backward (colour head, opacity head, trunk; weight gradients into LDS accumulators flushed once per workgroup).
// One loop over the levels follows with the lane's d feat: run-merged fp32 atomics into grad_table (hg_table_grad); `on` is false for
// lanes past S and for masked samples; no point gradient is formed.  The encoding gradient is accumulated per lane over the chunks,
// summed in a fixed order through the staging tile and STORED.  It reads nothing the forward wrote except chunk_nlt.
// 64-bit entry offsets throughout; no workspace; nothing but the caller's buffers is written.
#include "lp_column_mlp.h"
#include "lp_generic_decode.h"
#include "lp_hash_levels.h"
#include "lp_wave.h"

namespace lp {

namespace {

// what both kernels read of the rays and of the samples
struct HrRays {
  const float *origins, *directions, *depths, *deltas;
  int32_t S, n_chunks;
};

struct HrFwdArgs {
  LpHashGridArgs g;  // layout, table, grid_idx, flags (no points: they are formed in registers)
  HrRays rays;
  LpMlp trunk, opacity, color;
  const float* mlp_params;
  const float* encoding;
  const float* scaffold;
  LpGrid scaffold_shape;
  float *ray_length, *neg_log_t, *feature, *weights, *chunk_nlt;
  int32_t encoding_dim, color_chn;
  float gain;
  int32_t maxw;  // rows of one activation tile
};
static_assert(sizeof(HrFwdArgs) <= 4096, "a kernel's argument block has at most 4 KB");

// the ray of workgroup-uniform row r with its batch element in an SGPR: the level bases formed from it are scalars
LP_DEV Ray uniform_ray(const LpHashGridArgs& g, const HrRays& rays, int64_t r) {
  const int b = __builtin_amdgcn_readfirstlane(clamp_batch(g.grid_idx[r], g.batch));
  return sample_ray(rays.origins, rays.directions, r, b);
}

// dynamic LDS: activation tiles [maxw][64] -- two, or three with the colour head
template <bool OPACITY_ONLY>
__global__ void __launch_bounds__(SC_WAVE) hash_render_fwd(const HrFwdArgs s) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const LpHashGridArgs& g = s.g;
  const int lane = threadIdx.x;
  const int64_t r = blockIdx.x;
  const int S = s.rays.S;
  const int64_t base = r * S;
  const Ray ray = uniform_ray(g, s.rays, r);
  const bool mask = g.mask_out_of_bounds != 0;
  const bool contract = g.contract_coords != 0;
  const int C = g.n_levels * g.features_per_level;
  const int Cc = s.color_chn;
  const float* e = OPACITY_ONLY ? nullptr : s.encoding + r * s.encoding_dim;
  float carry = 0.0f, len = 0.0f;
  float facc[2] = {0.0f, 0.0f};  // lane c: channels c and 64 + c of the feature sums

  for (int k = 0; k < s.rays.n_chunks; ++k) {
    const int64_t sm = (int64_t)k * 64 + lane;  // (64-bit: the last chunk of a ray of nearly 2^31 samples ends beyond it)
    const bool in = sm < S;
    const int64_t at = base + (in ? sm : 0);
    const float dp = s.rays.depths[at];
    const float dl = s.rays.deltas[at];
    float x, y, z;
    sample_point(ray, dp, contract, x, y, z);
    const HgPoint pt = hg_point_at(ray, x, y, z, mask);
    float occ = 1.0f;
    if (s.scaffold) occ = scaffold_lookup(s.scaffold, s.scaffold_shape, ray.b, x, y, z);

    // ---- the field: the body of hash_points_fwd ----
    float* cur = lds + lane;
    float* nxt = lds + s.maxw * SC_WAVE + lane;
    hp_features<SC_WAVE>(g, pt, cur);
    if (s.trunk.n_layers == 0) {  // the heads read ReLU(features)
      for (int c = 0; c < C; ++c) cur[c * SC_WAVE] = fmaxf(cur[c * SC_WAVE], 0.0f);
    }
    int hw = C;  // width of the heads' input
    for (int l = 0; l < s.trunk.n_layers; ++l) {
      sc_dense(sc_const(mlp_w(s.mlp_params, s.trunk, l)), sc_const(mlp_b(s.mlp_params, s.trunk, l)), s.trunk.dims[l], s.trunk.dims[l + 1],
               s.trunk.dims[l + 1], cur, nxt, true);
      hw = s.trunk.dims[l + 1];
      float* t = cur;
      cur = nxt;
      nxt = t;
    }
    float* cin = lds + 2 * s.maxw * SC_WAVE + lane;  // the colour head's input (third tile; not there when OPACITY_ONLY)
    if (!OPACITY_ONLY) {
      for (int c = 0; c < hw; ++c) cin[c * SC_WAVE] = cur[c * SC_WAVE] + e[c];
    }
    for (int l = 0; l < s.opacity.n_layers; ++l) {
      const bool last = l == s.opacity.n_layers - 1;
      sc_dense(sc_const(mlp_w(s.mlp_params, s.opacity, l)), sc_const(mlp_b(s.mlp_params, s.opacity, l)), s.opacity.dims[l],
               s.opacity.dims[l + 1], last ? 1 : s.opacity.dims[l + 1], cur, nxt, !last);
      float* t = cur;
      cur = nxt;
      nxt = t;
    }
    const float opacity = s.gain * softplus_f(cur[0]) * occ;
    if (!OPACITY_ONLY) {
      cur = cin;  // (both other tiles are free now)
      for (int l = 0; l < s.color.n_layers; ++l) {
        const bool last = l == s.color.n_layers - 1;
        sc_dense(sc_const(mlp_w(s.mlp_params, s.color, l)), sc_const(mlp_b(s.mlp_params, s.color, l)), s.color.dims[l], s.color.dims[l + 1],
                 last ? Cc : s.color.dims[l + 1], cur, nxt, !last);
        float* t = cur;
        cur = nxt;
        nxt = t;
      }
    }

    // ---- compositing: the scan of composite_fwd ----
    const float od = in ? opacity * dl : 0.0f;
    const float incl = wave_scan(od, lane);
    const float up = __shfl_up(incl, 1, 64);
    const float nlt = carry + (lane > 0 ? up : 0.0f);  // -log T in front of the sample
    const float w = in ? expf(-nlt) * (-expm1f(-od)) : 0.0f;
    len += w * dp;
    if (s.weights && in) s.weights[at] = w;
    if (s.chunk_nlt && lane == 0) s.chunk_nlt[r * s.rays.n_chunks + k] = carry;
    carry += __shfl(incl, 63, 64);
    if (!OPACITY_ONLY) {
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
  }
  len = wave_sum(len);
  if (lane == 0) {
    if (s.ray_length) s.ray_length[r] = len;
    if (s.neg_log_t) s.neg_log_t[r] = carry;
  }
  if (!OPACITY_ONLY) {
    if (lane < Cc) s.feature[r * Cc + lane] = facc[0];
    if (lane + 64 < Cc) s.feature[r * Cc + lane + 64] = facc[1];
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------------------------------------

struct HrBwdArgs {
  GenArgs ga;        // the decoder and its parameter gradient in the generic Renderer's argument block (grid-list: channels only)
  LpHashGridArgs g;  // layout, table, grid_idx, flags; grad_table: result or NULL
  HrRays rays;
  const float* chunk_nlt;
  const float *g_len, *g_nlt, *g_feat, *g_w;
  float* grad_encoding;    // [n_rays, enc_dim], written (ga.a.grad_encoding stays NULL: nothing is added atomically)
  int32_t rays_per_block;  // consecutive rays of one workgroup
  int32_t color;           // the colour head takes part (g_feat given)
  int32_t enc_dim;         // columns of grad_encoding (ga.a.rays.encoding_dim is 0 without the colour head)
};
static_assert(sizeof(HrBwdArgs) <= 4096, "a kernel's argument block has at most 4 KB");

// one level of the backward: d = the lane's d feat[l F ..] (used when `on`); `level`: the level's first float in grad_table (a scalar)
template <int F>
LP_DEV void hr_level_b(float* level, const HgPoint& pt, const HgLevel& lv, const float* d, bool on, int lane) {
  HgRow<F> dl;
#pragma unroll
  for (int c = 0; c < F; ++c) dl.v[c] = on ? d[c] : 0.0f;
  const HgCell cell = hg_cell(pt, lv);
  hg_table_grad<F>(level, cell, lv, dl, on, hg_run_ray(cell, on, lane));
}

// dynamic LDS: Xs[64][ld] | Ys[64][ld] | (LDS_ACC) the weight-gradient accumulators [n_mlp_params]
template <int ACT_CAP, bool LDS_ACC>
__global__ void __launch_bounds__(64) hash_render_bwd(const HrBwdArgs s) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const GenArgs& ga = s.ga;
  const LpRendererArgs& a = ga.a;
  const GenPlan& p = ga.p;
  const LpHashGridArgs& g = s.g;
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
  const bool contract = g.contract_coords != 0;
  const bool mask = g.mask_out_of_bounds != 0;
  const bool color = s.color != 0;  // wave-uniform
  const int C = a.grid.channels;    // L F
  const int F = g.features_per_level;
  const int hw = p.head_w;
  const int craw = color ? p.col[a.color.n_layers - 1] : 0;
  const int S = s.rays.S;
  const int n_chunks = s.rays.n_chunks;

  for (int t = 0; t < s.rays_per_block; ++t) {
    const int64_t r = (int64_t)blockIdx.x * s.rays_per_block + t;
    if (r >= a.rays.n_rays) break;  // wave-uniform
    const Ray ray = uniform_ray(g, s.rays, r);
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

    for (int k = n_chunks - 1; k >= 0; --k) {
      const int64_t sm = (int64_t)k * 64 + lane;  // (64-bit: the last chunk of a ray of nearly 2^31 samples ends beyond it)
      const bool live = sm < S;
      const int64_t at = base + (live ? sm : 0);  // (a lane past the end recomputes sample 0 and contributes nothing)
      const float dp = s.rays.depths[at];
      const float dl = s.rays.deltas[at];
      float x, y, z;
      sample_point(ray, dp, contract, x, y, z);
      const HgPoint pt = hg_point_at(ray, x, y, z, mask);
      float occ = 1.0f;
      if (a.scaffold) occ = scaffold_lookup(a.scaffold, a.scaffold_shape, ray.b, x, y, z);
      hp_features<1>(g, pt, act + p.x0);
      const float raw = color ? decode_gathered(ga, enc, act, Xs, lane) : decode_opacity_gathered(ga, act, Xs, lane);

      // ---- compositing backward: the chunk step of composite_bwd ----
      const float o = a.gain * softplus_f(raw) * occ;
      const float od = live ? o * dl : 0.0f;
      const float c0 = s.chunk_nlt[r * n_chunks + k];
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

      // ---- the decoder backward: the body of hash_points_bwd ----
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
      // trunk output gradient = colour-input grad + opacity-input grad, through the ReLU
      for (int c = 0; c < hw; ++c) {
        const float gsum = dhead[c] + dx[c];
        dy[c] = (act[p.op_in + c] > 0.0f) ? gsum : 0.0f;
      }
      if (a.trunk.n_layers > 0) {
        const LpMlp& m = a.trunk;
        mlp_backward<LDS_ACC>(a.mlp_params, ga.stage_ld, m, m.dims[m.n_layers], p.x0, p.trunk, act, dy, dx, gparams, Xs, Ys, lane, live);
      } else {
        for (int c = 0; c < C; ++c) dx[c] = dy[c];
      }
      // ---- the levels: dx = d feat; the level's base in grad_table is a scalar ----
      if (g.grad_table) {
        const bool on = live && pt.inside;
        for (int l = 0; l < g.n_levels; ++l) {
          const HgLevel lv = hg_level(g, l);
          float* level = g.grad_table + hg_base(g, ray.b, lv, F);
          const float* d = dx + l * F;
          switch (F) {
            case 1: hr_level_b<1>(level, pt, lv, d, on, lane); break;
            case 2: hr_level_b<2>(level, pt, lv, d, on, lane); break;
            case 4: hr_level_b<4>(level, pt, lv, d, on, lane); break;
            default: hr_level_b<8>(level, pt, lv, d, on, lane); break;
          }
        }
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

// ---------------------------------------------------------------------------------------------------------------------------
// host side (`a` checked by lp_api.hip)
// ---------------------------------------------------------------------------------------------------------------------------

constexpr int64_t HR_BWD_BLOCKS = 2048;  // workgroups a large backward is cut into, as render_samples_bwd

HrRays rays_view(const LpHashRenderArgs& a) {
  return {a.origins, a.directions, a.depths, a.deltas, a.n_samples, lp_render_samples_chunks(a.n_samples)};
}

// the generic Renderer's argument block of the decoder: no grid-list, `channels` features
void decoder_view(const LpHashRenderArgs& a, bool color, LpRendererArgs& ra) {
  ra = LpRendererArgs{};
  ra.rays.n_rays = a.n_rays;
  ra.rays.grid_idx = a.grid_idx;
  ra.rays.encoding = a.encoding;
  ra.rays.encoding_dim = color ? a.encoding_dim : 0;
  ra.grid.channels = a.n_levels * a.features_per_level;
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
}

int forward_launch(const LpHashRenderArgs& a, hipStream_t stream) {
  HrFwdArgs s;
  s.g = hash_render_view(a);
  s.rays = rays_view(a);
  const bool opacity_only = a.feature == nullptr;
  s.trunk = a.trunk, s.opacity = a.opacity, s.color = a.color;
  s.mlp_params = a.mlp_params;
  s.encoding = a.encoding;
  s.scaffold = a.scaffold;
  s.scaffold_shape = a.scaffold_shape;
  s.ray_length = a.ray_length, s.neg_log_t = a.neg_log_t, s.feature = a.feature, s.weights = a.weights, s.chunk_nlt = a.chunk_nlt;
  s.encoding_dim = a.encoding_dim;
  s.color_chn = a.color_chn;
  s.gain = a.gain;
  int maxw = a.n_levels * a.features_per_level;
  const LpMlp* ms[3] = {&a.trunk, &a.opacity, &a.color};
  for (int k = 0; k < (opacity_only ? 2 : 3); ++k)
    for (int l = 0; l <= ms[k]->n_layers && ms[k]->n_layers > 0; ++l) maxw = ms[k]->dims[l] > maxw ? ms[k]->dims[l] : maxw;
  s.maxw = maxw;
  const size_t lds = (size_t)(opacity_only ? 2 : 3) * maxw * SC_WAVE * sizeof(float);  // <= 96 KB (LP_MAX_WIDTH 128)
  // (one workgroup per ray: lp_api.hip keeps n_rays * n_samples, hence n_rays, below 2^31)
  unsigned blocks;
  if (int rc = launch_blocks("lp_hash_render_forward", a.n_rays, 1, blocks)) return rc;
  const void* fn = opacity_only ? (const void*)hash_render_fwd<true> : (const void*)hash_render_fwd<false>;
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return set_error((int)e, "hipFuncSetAttribute: %s", hipGetErrorString(e));
  const dim3 gr(blocks), bl(SC_WAVE);
  if (opacity_only)
    hipLaunchKernelGGL((hash_render_fwd<true>), gr, bl, lds, stream, s);
  else
    hipLaunchKernelGGL((hash_render_fwd<false>), gr, bl, lds, stream, s);
  return check_launch("hash_render_fwd");
}

int backward_launch(const LpHashRenderArgs& a, hipStream_t stream) {
  if (!a.grad_ray_length && !a.grad_neg_log_t && !a.grad_feature && !a.grad_weights) return LP_OK;  // every result is zero
  HrBwdArgs s;
  const bool color = a.grad_feature != nullptr;
  decoder_view(a, color, s.ga.a);
  const LpRendererArgs& ra = s.ga.a;
  s.g = hash_render_view(a);
  s.rays = rays_view(a);
  const int total = make_plan(ra, s.ga.p);  // (<= 1024: lp_api.hip)
  s.ga.stage_ld = generic_stage_ld(ra);
  s.ga.relu_dump = nullptr;
  s.ga.dump_words = s.ga.dump_wps = 0;
  s.chunk_nlt = a.chunk_nlt;
  s.g_len = a.grad_ray_length, s.g_nlt = a.grad_neg_log_t, s.g_feat = a.grad_feature, s.g_w = a.grad_weights;
  s.grad_encoding = a.grad_encoding;
  s.color = color ? 1 : 0;
  s.enc_dim = a.encoding_dim;
  const size_t stage_bytes = (size_t)128 * s.ga.stage_ld * sizeof(float);
  const size_t param_bytes = (size_t)a.n_mlp_params * sizeof(float);
  const bool lds_acc = a.grad_mlp_params && (stage_bytes + param_bytes <= 96 * 1024);
  s.ga.lds_param_accum = lds_acc ? 1 : 0;
  const size_t lds = stage_bytes + (lds_acc ? param_bytes : 0);
  int64_t rpb;
  workgroup_count(a.n_rays, HR_BWD_BLOCKS, rpb);  // (n_rays < 2^31)
  s.rays_per_block = (int32_t)rpb;
  unsigned blocks;
  if (int rc = launch_blocks("lp_hash_render_backward", a.n_rays, rpb, blocks)) return rc;
#define LP_LAUNCH_HR_BWD(CAP, ACC)                                                                                                    \
  do {                                                                                                                                \
    hipError_t e = hipFuncSetAttribute((const void*)hash_render_bwd<CAP, ACC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    if (e != hipSuccess) return set_error((int)e, "hipFuncSetAttribute: %s", hipGetErrorString(e));                                   \
    hipLaunchKernelGGL((hash_render_bwd<CAP, ACC>), dim3(blocks), dim3(64), lds, stream, s);                                          \
  } while (0)
  if (total <= 256) {
    if (lds_acc) LP_LAUNCH_HR_BWD(256, true); else LP_LAUNCH_HR_BWD(256, false);
  } else {
    if (lds_acc) LP_LAUNCH_HR_BWD(1024, true); else LP_LAUNCH_HR_BWD(1024, false);
  }
#undef LP_LAUNCH_HR_BWD
  return check_launch("hash_render_bwd");
}

}  // namespace

// the layout, the table and the flags as the level functions (and the layout check of lp_api.hip) read them; n_pts = n_samples
LpHashGridArgs hash_render_view(const LpHashRenderArgs& a) {
  LpHashGridArgs g = {};
  g.table = a.table;
  g.grad_table = a.grad_table;
  g.grid_idx = a.grid_idx;
  g.entries = a.entries;
  g.n_rays = a.n_rays;
  g.n_pts = a.n_samples;
  for (int l = 0; l < LP_HASH_MAX_LEVELS; ++l) {
    g.offset[l] = a.offset[l];
    g.resolution[l] = a.resolution[l];
    g.size[l] = a.size[l];
    g.hashed[l] = a.hashed[l];
  }
  g.batch = a.batch;
  g.features_per_level = a.features_per_level;
  g.n_levels = a.n_levels;
  g.mask_out_of_bounds = a.mask_out_of_bounds;
  g.contract_coords = a.contract_coords;
  return g;
}

int hash_render_backward_total_width(const LpHashRenderArgs& a) {
  LpRendererArgs ra;
  decoder_view(a, a.grad_feature != nullptr, ra);
  GenPlan p;
  return make_plan(ra, p);
}

// `a` checked by lp_api.hip: n_rays > 0, n_samples >= 1, n_rays * n_samples < 2^31
int hash_render_launch(const LpHashRenderArgs& a, bool backward, hipStream_t stream) {
  return backward ? backward_launch(a, stream) : forward_launch(a, stream);
}

const char* build_info_hash_render() {
  return "{\"forward\": \"one wavefront per ray, lanes = samples in chunks of 64: hash-grid levels with scalar level bases, the decoder "
         "of the hash-points forward (LDS column tiles, fp32 FMA, no scratch) and the compositing scan in one launch; fixed-order "
         "sums\", \"backward\": \"one wavefront per ray, chunks far to near from the saved per-chunk -log T: recompute, decoder backward, "
         "run-merged fp32 atomics into the table; encoding gradient stored per ray, no atomics\"}";
}

}  // namespace lp

// lp_kplanes_render.hip -- a space-time plane field (K-Planes / HexPlane; without time planes the Hadamard tri-plane) rendered along
// rays at caller-given sample depths: encoding, decoder and compositing in one launch, forward and backward (C ABI
// lp_kplanes_render_forward / lp_kplanes_render_backward of include/lightplane_hip_kplanes_render.h, which holds the definition).  It
// is the product of lp_kplanes_points.hip (the field at points) and lp_hash_render.hip (a field decoded and composited along a ray),
// and replaces the chain ray_samples -> kplanes_points -> composite without its [n_rays, n_samples] tensors.
//
// Both kernels: one wavefront = one workgroup works on ONE RAY at a time, lanes = samples, chunks of 64 with the -log T carried
// between them.  What the ray-major split buys on planes:
//   * the batch element b is wave-uniform (readfirstlane), so every plane's base b rows + offset[s][j] is a scalar;
//   * with one timestamp per ray the time-axis cell (vertex, fraction) of every scale is formed ONCE PER RAY (kr_time_cells: a
//     uniform loop over the scales leaves them in 16 words of LDS, every lane reads them as a broadcast) instead of per lane and chunk;
//   * a ray's consecutive samples are neighbours in every plane: the run-merged walk of the backward (kpp_walk) meets long runs.
//
// Forward, kplanes_render_fwd<P, OPACITY_ONLY>, per chunk:
//   1  lane = sample forms its point in registers (sample_point: the arithmetic of ray_samples / importance_samples, whose points the
//      chain reads back), the mask and the scaffold's value, once;
//   2  per scale it leaves geo[64][KP_LD(P)] (kp_tile_store) in the ping-pong tile, and lanes = channels gather whole plane rows into
//      rows s C .. of the feature tile (kpp_gather, lp_kplanes_tile.h: the body of the points kernel, the same bits);
//   3  lane = sample runs the decoder (sc_dense, weights through sc_const: scalar loads that stay scalar behind the chunk before's
//      stores); 4  the scan of composite_fwd and the colour fold of render_samples_fwd.
//   No private array and no atomics: every result is bit-reproducible.  A lane past S works on sample 0 and contributes nothing.
//
// LDS of the forward: time cells [16 words] | feature tile [rows0][64] | ping-pong tile [rows1][64] | colour-input tile [head_w][64]
// (not there when OPACITY_ONLY).  Each tile has the rows of the widest thing it ever holds -- kr_tile_rows() walks the decoder the way
// the kernel does: the feature tile holds S C features and every second layer output from there on, the ping-pong tile the geometry
// (4 P + 1 rows) and the other layer outputs, the colour-input tile head_w rows only (the colour head's first layer writes into the
// feature tile, its later layers alternate between the two other tiles; a head's last layer counts with the rows it stores, 1 or
// color_chn).  S C = 128 with a hidden-32 decoder: 128 + 32 + 32 rows = 48 KB (+ 64 bytes), where three tiles of the widest width
// take 96 KB.
//
// Backward, kplanes_render_bwd<P, ACT_CAP, LDS_ACC>: a workgroup takes a run of consecutive rays and walks each ray's chunks far ->
// near.  LDS: Xs[64][ld] | Ys[64][ld] (ld = max(widest layer + 1, 4 P + 1)) | time cells [16] | the weight-gradient accumulators
// when they fit.  Per chunk: geometry into Ys, kpp_gather into Xs as [sample][ld], the lane copies its row into act + p.x0;
// decode_gathered / decode_opacity_gathered; T from chunk_nlt plus the scan inside the chunk, the suffix sums from wave_rscan with a
// carry; mlp_backward through the colour head, the opacity head and the trunk; d feat is staged into Xs (zeros for a masked sample or
// a lane past S), the geometry goes into Ys again and kpp_walk (no point gradient) adds whole rows to grad_planes with fp32 atomics,
// only where a plane's base row changes.  The encoding gradient is accumulated per lane over the chunks, summed in a fixed order
// through the staging tile and STORED.  It reads nothing the forward wrote except chunk_nlt.  Lanes past S and masked samples take
// part in barriers and shuffles and add nothing; rows no sample touches stay exactly 0.  64-bit row offsets throughout; no workspace.
// The private arrays of the generic backward (and their scratch) are inherited.
#include "lp_column_mlp.h"
#include "lp_generic_decode.h"
#include "lp_kplanes_tile.h"
#include "lp_wave.h"

namespace lp {

namespace {

constexpr int KR_TC = 2 * LP_KPLANES_MAX_SCALES;  // words of the time cells: (vertex, fraction) per scale

// what both kernels read of the rays and of the samples
struct KrRays {
  const float *origins, *directions, *depths, *deltas;
  int32_t S, n_chunks;
};

// the ray of workgroup-uniform row r with its batch element in an SGPR: the plane bases formed from it are scalars
LP_DEV Ray kr_uniform_ray(const LpKPlanesArgs& g, const KrRays& rays, int64_t r) {
  const int b = __builtin_amdgcn_readfirstlane(clamp_batch(g.grid_idx[r], g.batch));
  return sample_ray(rays.origins, rays.directions, r, b);
}

// one timestamp per ray: the time-axis cell of every scale, once per ray, into tc[2 s] (vertex) and tc[2 s + 1] (fraction).  Every
// lane of the wave calls this; the barriers fence the cells of the ray before.
template <int P>
LP_DEV void kr_time_cells(const LpKPlanesArgs& g, int64_t r, int lane, float* tc) {
  if constexpr (P == 6) {
    if (!g.time_per_point) {
      __syncthreads();
      const float t = g.times[r];
      for (int s = 0; s < g.n_scales; ++s) {
        const KpAxis ax = kp_axis(t, g.temporal[s]);
        if (lane == 0) {
          tc[2 * s] = __int_as_float(ax.i);
          tc[2 * s + 1] = ax.f;
        }
      }
      __syncthreads();
    }
  }
}

// the sample's cell on scale s: kp_cell, with the time axis from the ray's cells where the timestamp is the ray's
template <int P>
LP_DEV KpCell kr_cell(const LpKPlanesArgs& g, const KpPoint& pt, int s, const float* tc) {
  KpCell c;
  c.n = g.spatial[s];
  c.ax[0] = kp_axis(pt.x, c.n);
  c.ax[1] = kp_axis(pt.y, c.n);
  c.ax[2] = kp_axis(pt.z, c.n);
  c.ax[3] = KpAxis{0, 0.0f, false};
  if constexpr (P == 6) {
    if (g.time_per_point) {
      c.ax[3] = kp_axis(pt.t, g.temporal[s]);
    } else {
      c.ax[3].i = __float_as_int(tc[2 * s]);
      c.ax[3].f = tc[2 * s + 1];
    }
  }
  return c;
}

// sample `at` (< n_rays * S) of `ray` at depth dp: where the planes are sampled, its timestamp and whether the mask keeps it
template <int P>
LP_DEV KpPoint kr_point(const LpKPlanesArgs& g, const Ray& ray, float dp, int64_t at) {
  KpPoint pt;
  pt.ray = ray;
  sample_point(ray, dp, g.contract_coords != 0, pt.x, pt.y, pt.z);
  pt.inside = !(g.mask_out_of_bounds != 0 && !point_in_bounds(pt.x, pt.y, pt.z));
  pt.t = 0.0f;
  if constexpr (P == 6) {
    if (g.time_per_point) pt.t = g.times[at];
  }
  return pt;
}

struct KrFwdArgs {
  LpKPlanesArgs g;  // layout, planes, times, grid_idx, flags (no points: they are formed in registers)
  KrRays rays;
  LpMlp trunk, opacity, color;
  const float* mlp_params;
  const float* encoding;
  const float* scaffold;
  LpGrid scaffold_shape;
  float *ray_length, *neg_log_t, *feature, *weights, *chunk_nlt;
  int32_t encoding_dim, color_chn;
  float gain;
  int32_t rows0, rows1;  // rows of the feature tile and of the ping-pong tile (kr_tile_rows); the colour-input tile follows them
  int32_t lanes_log;     // log2(C / 4): lanes per sample of the gather
};
static_assert(sizeof(KrFwdArgs) <= 4096, "a kernel's argument block has at most 4 KB");

template <int P, bool OPACITY_ONLY>
__global__ void __launch_bounds__(SC_WAVE) kplanes_render_fwd(const KrFwdArgs s) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const LpKPlanesArgs& g = s.g;
  const int lane = threadIdx.x;
  const int64_t r = blockIdx.x;
  const int S = s.rays.S;
  const int64_t base = r * S;
  const Ray ray = kr_uniform_ray(g, s.rays, r);
  const int C = g.n_scales * g.channels;
  const int Cc = s.color_chn;
  const float* e = OPACITY_ONLY ? nullptr : s.encoding + r * s.encoding_dim;
  float* tc = lds;
  float* tile0 = lds + KR_TC;
  float* tile1 = tile0 + s.rows0 * SC_WAVE;
  float* tilec = tile1 + s.rows1 * SC_WAVE;
  kr_time_cells<P>(g, r, lane, tc);
  float carry = 0.0f, len = 0.0f;
  float facc[2] = {0.0f, 0.0f};  // lane c: channels c and 64 + c of the feature sums

  for (int k = 0; k < s.rays.n_chunks; ++k) {
    const int64_t sm = (int64_t)k * 64 + lane;  // (64-bit: the last chunk of a ray of nearly 2^31 samples ends beyond it)
    const bool in = sm < S;
    const int64_t at = base + (in ? sm : 0);
    const float dp = s.rays.depths[at];
    const float dl = s.rays.deltas[at];
    const KpPoint pt = kr_point<P>(g, ray, dp, at);
    float occ = 1.0f;
    if (s.scaffold) occ = scaffold_lookup(s.scaffold, s.scaffold_shape, ray.b, pt.x, pt.y, pt.z);

    // ---- the field: geometry by lane = sample, gather by lanes = channels (the body of kplanes_points_fwd) ----
    __syncthreads();  // (the chunk before has left the tiles)
    for (int sc = 0; sc < g.n_scales; ++sc) {
      kp_tile_store<P>(g, kr_cell<P>(g, pt, sc, tc), ray.b, sc, in && pt.inside, tile1 + lane * KP_LD(P));
      __syncthreads();
      kpp_gather<P>(g, tile1, sc, s.lanes_log, lane, tile0, 1, SC_WAVE);
      __syncthreads();
    }
    float* cur = tile0 + lane;
    float* nxt = tile1 + lane;
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
    if (!OPACITY_ONLY) {
      float* cin = tilec + lane;
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
      // both other tiles are free now: layer l of the colour head writes into the feature tile (l even) or the ping-pong tile (l odd)
      cur = tilec + lane;
      for (int l = 0; l < s.color.n_layers; ++l) {
        const bool last = l == s.color.n_layers - 1;
        nxt = ((l & 1) ? tile1 : tile0) + lane;
        sc_dense(sc_const(mlp_w(s.mlp_params, s.color, l)), sc_const(mlp_b(s.mlp_params, s.color, l)), s.color.dims[l], s.color.dims[l + 1],
                 last ? Cc : s.color.dims[l + 1], cur, nxt, !last);
        cur = nxt;
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

struct KrBwdArgs {
  GenArgs ga;       // the decoder and its parameter gradient in the generic Renderer's argument block (grid-list: channels only)
  LpKPlanesArgs g;  // layout, planes, times, grid_idx, flags; grad_planes: result or NULL (grad_points stays NULL)
  KrRays rays;
  const float* chunk_nlt;
  const float *g_len, *g_nlt, *g_feat, *g_w;
  float* grad_encoding;    // [n_rays, enc_dim], written (ga.a.grad_encoding stays NULL: nothing is added atomically)
  int32_t rays_per_block;  // consecutive rays of one workgroup
  int32_t color;           // the colour head takes part (g_feat given)
  int32_t enc_dim;         // columns of grad_encoding (ga.a.rays.encoding_dim is 0 without the colour head)
  int32_t lanes_log;       // log2(C / 4): lanes per sample of the gather
  int32_t cw_log;          // log2(C): lanes of a group of the walk
};
static_assert(sizeof(KrBwdArgs) <= 4096, "a kernel's argument block has at most 4 KB");

// dynamic LDS: Xs[64][ld] | Ys[64][ld] | time cells [KR_TC] | (LDS_ACC) the weight-gradient accumulators [n_mlp_params]
template <int P, int ACT_CAP, bool LDS_ACC>
__global__ void __launch_bounds__(64) kplanes_render_bwd(const KrBwdArgs s) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const GenArgs& ga = s.ga;
  const LpRendererArgs& a = ga.a;
  const GenPlan& p = ga.p;
  const LpKPlanesArgs& g = s.g;
  const int lane = threadIdx.x;
  const int ld = ga.stage_ld;  // >= S C + 1 and >= KP_LD(P)

  float* Xs = lds;
  float* Ys = lds + 64 * ld;
  float* tc = lds + 128 * ld;
  float* gparams_lds = tc + KR_TC;
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
  const bool color = s.color != 0;  // wave-uniform
  const int C = a.grid.channels;    // S C
  const int hw = p.head_w;
  const int craw = color ? p.col[a.color.n_layers - 1] : 0;
  const int S = s.rays.S;
  const int n_chunks = s.rays.n_chunks;

  for (int t = 0; t < s.rays_per_block; ++t) {
    const int64_t r = (int64_t)blockIdx.x * s.rays_per_block + t;
    if (r >= a.rays.n_rays) break;  // wave-uniform
    const Ray ray = kr_uniform_ray(g, s.rays, r);
    kr_time_cells<P>(g, r, lane, tc);
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
      const KpPoint pt = kr_point<P>(g, ray, dp, at);
      const bool on = live && pt.inside;
      float occ = 1.0f;
      if (a.scaffold) occ = scaffold_lookup(a.scaffold, a.scaffold_shape, ray.b, pt.x, pt.y, pt.z);
      // ---- recompute: geometry by lane = sample, gather by lanes = channels into Xs[sample][ld], back to lane = sample ----
      __syncthreads();  // (the chunk before has left the tiles)
      for (int sc = 0; sc < g.n_scales; ++sc) {
        kp_tile_store<P>(g, kr_cell<P>(g, pt, sc, tc), ray.b, sc, on, Ys + lane * KP_LD(P));
        __syncthreads();
        kpp_gather<P>(g, Ys, sc, s.lanes_log, lane, Xs, ld, 1);
        __syncthreads();
      }
      for (int c = 0; c < C; ++c) act[p.x0 + c] = Xs[lane * ld + c];
      __syncthreads();
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

      // ---- the decoder backward: the body of kplanes_points_bwd ----
      if (color) {
        for (int c = 0; c < Cc; ++c) {
          const float sg = sigmoid_f(act[craw + c]);
          dy[c] = live ? w * gf[c] * occ * sg * (1.0f - sg) : 0.0f;
        }
        mlp_backward<LDS_ACC>(a.mlp_params, ld, a.color, Cc, p.col_in, p.col, act, dy, dx, gparams, Xs, Ys, lane, live);
        for (int c = 0; c < hw; ++c) dhead[c] = dx[c];
        if (s.grad_encoding)
          for (int c = 0; c < E; ++c) genc[c] += live ? dx[c] : 0.0f;
      } else {
        for (int c = 0; c < hw; ++c) dhead[c] = 0.0f;
      }
      dy[0] = d_raw_op;
      mlp_backward<LDS_ACC>(a.mlp_params, ld, a.opacity, 1, p.op_in, p.op, act, dy, dx, gparams, Xs, Ys, lane, live);
      // trunk output gradient = colour-input grad + opacity-input grad, through the ReLU
      for (int c = 0; c < hw; ++c) {
        const float gsum = dhead[c] + dx[c];
        dy[c] = (act[p.op_in + c] > 0.0f) ? gsum : 0.0f;
      }
      if (a.trunk.n_layers > 0) {
        const LpMlp& m = a.trunk;
        mlp_backward<LDS_ACC>(a.mlp_params, ld, m, m.dims[m.n_layers], p.x0, p.trunk, act, dy, dx, gparams, Xs, Ys, lane, live);
      } else {
        for (int c = 0; c < C; ++c) dx[c] = dy[c];
      }
      // ---- the planes: dx = d feat goes to lanes = channels through Xs; groups of C lanes walk consecutive samples of the ray ----
      if (g.grad_planes) {
        __syncthreads();
        stage(Xs, ld, lane, dx, C, !on);
        for (int sc = 0; sc < g.n_scales; ++sc) {
          kp_tile_store<P>(g, kr_cell<P>(g, pt, sc, tc), ray.b, sc, on, Ys + lane * KP_LD(P));
          __syncthreads();
          kpp_walk<P>(g, Ys, Xs, ld, sc, s.cw_log, lane, nullptr);
          __syncthreads();
        }
      }
    }

    // the ray's encoding gradient: the lanes' sums through the staging tile, lanes = channels over its 64 rows in ascending order
    if (s.grad_encoding) {
      float* out = s.grad_encoding + r * s.enc_dim;
      if (color) {
        __syncthreads();
        stage(Xs, ld, lane, genc, E, false);
        __syncthreads();
        for (int c = lane; c < E; c += 64) out[c] = column_sum(Xs + c, ld, 0.0f);
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

constexpr int64_t KR_BWD_BLOCKS = 2048;  // workgroups a large backward is cut into, as hash_render_bwd

int kr_log2(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

KrRays rays_view(const LpKPlanesRenderArgs& a) {
  return {a.origins, a.directions, a.depths, a.deltas, a.n_samples, lp_render_samples_chunks(a.n_samples)};
}

// rows of the forward's three tiles: the decoder walked the way kplanes_render_fwd walks it, every tile with the most rows it is
// ever given.  rows[0]: feature tile, rows[1]: ping-pong tile, rows[2]: colour-input tile (0 without the colour head)
void kr_tile_rows(const LpKPlanesRenderArgs& a, bool color, int rows[3]) {
  const auto grow = [&](int tile, int n) { rows[tile] = n > rows[tile] ? n : rows[tile]; };
  rows[0] = a.n_scales * a.channels;
  rows[1] = KP_LD(a.n_planes);
  rows[2] = 0;
  int cur = 0, hw = rows[0];
  for (int l = 0; l < a.trunk.n_layers; ++l) {
    hw = a.trunk.dims[l + 1];
    grow(cur ^= 1, hw);
  }
  for (int l = 0; l < a.opacity.n_layers; ++l) grow(cur ^= 1, l == a.opacity.n_layers - 1 ? 1 : a.opacity.dims[l + 1]);
  if (color) {
    rows[2] = hw;
    for (int l = 0; l < a.color.n_layers; ++l) grow(l & 1, l == a.color.n_layers - 1 ? a.color_chn : a.color.dims[l + 1]);
  }
}

// the generic Renderer's argument block of the decoder: no grid-list, `channels` features
void decoder_view(const LpKPlanesRenderArgs& a, bool color, LpRendererArgs& ra) {
  ra = LpRendererArgs{};
  ra.rays.n_rays = a.n_rays;
  ra.rays.grid_idx = a.grid_idx;
  ra.rays.encoding = a.encoding;
  ra.rays.encoding_dim = color ? a.encoding_dim : 0;
  ra.grid.channels = a.n_scales * a.channels;
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

int forward_launch(const LpKPlanesRenderArgs& a, hipStream_t stream) {
  KrFwdArgs s;
  s.g = kplanes_render_view(a);
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
  s.lanes_log = kr_log2(a.channels / 4);
  int rows[3];
  kr_tile_rows(a, !opacity_only, rows);
  s.rows0 = rows[0], s.rows1 = rows[1];
  // <= 96 KB + 64 bytes (three tiles of LP_MAX_WIDTH 128 rows); 48 KB + 64 bytes at S C = 128 with a hidden-32 decoder
  const size_t lds = ((size_t)(rows[0] + rows[1] + rows[2]) * SC_WAVE + KR_TC) * sizeof(float);
  // (one workgroup per ray: lp_api.hip keeps n_rays * n_samples, hence n_rays, below 2^31)
  unsigned blocks;
  if (int rc = launch_blocks("lp_kplanes_render_forward", a.n_rays, 1, blocks)) return rc;
#define LP_LAUNCH_KR_FWD(P, OO)                                                                                                        \
  do {                                                                                                                                 \
    hipError_t e = hipFuncSetAttribute((const void*)kplanes_render_fwd<P, OO>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    if (e != hipSuccess) return set_error((int)e, "hipFuncSetAttribute: %s", hipGetErrorString(e));                                    \
    hipLaunchKernelGGL((kplanes_render_fwd<P, OO>), dim3(blocks), dim3(SC_WAVE), lds, stream, s);                                      \
  } while (0)
  if (a.n_planes == 3) {
    if (opacity_only) LP_LAUNCH_KR_FWD(3, true); else LP_LAUNCH_KR_FWD(3, false);
  } else {
    if (opacity_only) LP_LAUNCH_KR_FWD(6, true); else LP_LAUNCH_KR_FWD(6, false);
  }
#undef LP_LAUNCH_KR_FWD
  return check_launch("kplanes_render_fwd");
}

int backward_launch(const LpKPlanesRenderArgs& a, hipStream_t stream) {
  if (!a.grad_ray_length && !a.grad_neg_log_t && !a.grad_feature && !a.grad_weights) return LP_OK;  // every result is zero
  KrBwdArgs s;
  const bool color = a.grad_feature != nullptr;
  decoder_view(a, color, s.ga.a);
  const LpRendererArgs& ra = s.ga.a;
  s.g = kplanes_render_view(a);
  s.rays = rays_view(a);
  const int total = make_plan(ra, s.ga.p);  // (<= 1024: lp_api.hip)
  const int geo = KP_LD(a.n_planes);        // the geometry tile [64][4 P + 1] lies in the second staging tile
  const int ld = generic_stage_ld(ra);
  s.ga.stage_ld = ld > geo ? ld : geo;
  s.ga.relu_dump = nullptr;
  s.ga.dump_words = s.ga.dump_wps = 0;
  s.chunk_nlt = a.chunk_nlt;
  s.g_len = a.grad_ray_length, s.g_nlt = a.grad_neg_log_t, s.g_feat = a.grad_feature, s.g_w = a.grad_weights;
  s.grad_encoding = a.grad_encoding;
  s.color = color ? 1 : 0;
  s.enc_dim = a.encoding_dim;
  s.lanes_log = kr_log2(a.channels / 4);
  s.cw_log = kr_log2(a.channels);
  const size_t stage_bytes = ((size_t)128 * s.ga.stage_ld + KR_TC) * sizeof(float);  // Xs, Ys and the time cells
  const size_t param_bytes = (size_t)a.n_mlp_params * sizeof(float);
  const bool lds_acc = a.grad_mlp_params && (stage_bytes + param_bytes <= 96 * 1024);
  s.ga.lds_param_accum = lds_acc ? 1 : 0;
  const size_t lds = stage_bytes + (lds_acc ? param_bytes : 0);
  int64_t rpb;
  workgroup_count(a.n_rays, KR_BWD_BLOCKS, rpb);  // (n_rays < 2^31)
  s.rays_per_block = (int32_t)rpb;
  unsigned blocks;
  if (int rc = launch_blocks("lp_kplanes_render_backward", a.n_rays, rpb, blocks)) return rc;
#define LP_LAUNCH_KR_BWD(P, CAP, ACC)                                                                                                       \
  do {                                                                                                                                      \
    hipError_t e = hipFuncSetAttribute((const void*)kplanes_render_bwd<P, CAP, ACC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    if (e != hipSuccess) return set_error((int)e, "hipFuncSetAttribute: %s", hipGetErrorString(e));                                         \
    hipLaunchKernelGGL((kplanes_render_bwd<P, CAP, ACC>), dim3(blocks), dim3(64), lds, stream, s);                                          \
  } while (0)
#define LP_LAUNCH_KR_BWD_P(P)                                                         \
  if (total <= 256) {                                                                 \
    if (lds_acc) LP_LAUNCH_KR_BWD(P, 256, true); else LP_LAUNCH_KR_BWD(P, 256, false);   \
  } else {                                                                            \
    if (lds_acc) LP_LAUNCH_KR_BWD(P, 1024, true); else LP_LAUNCH_KR_BWD(P, 1024, false); \
  }
  if (a.n_planes == 3) {
    LP_LAUNCH_KR_BWD_P(3)
  } else {
    LP_LAUNCH_KR_BWD_P(6)
  }
#undef LP_LAUNCH_KR_BWD_P
#undef LP_LAUNCH_KR_BWD
  return check_launch("kplanes_render_bwd");
}

}  // namespace

// the layout, the planes, the timestamps and the flags as the plane helpers (and the layout check of lp_api.hip) read them;
// n_pts = n_samples, no points
LpKPlanesArgs kplanes_render_view(const LpKPlanesRenderArgs& a) {
  LpKPlanesArgs g = {};
  g.planes = a.planes;
  g.grad_planes = a.grad_planes;
  g.times = a.times;
  g.grid_idx = a.grid_idx;
  g.rows = a.rows;
  g.n_rays = a.n_rays;
  g.n_pts = a.n_samples;
  for (int s = 0; s < LP_KPLANES_MAX_SCALES; ++s) {
    for (int j = 0; j < LP_KPLANES_MAX_PLANES; ++j) g.offset[s][j] = a.offset[s][j];
    g.spatial[s] = a.spatial[s];
    g.temporal[s] = a.temporal[s];
  }
  g.batch = a.batch;
  g.channels = a.channels;
  g.n_scales = a.n_scales;
  g.n_planes = a.n_planes;
  g.time_per_point = a.time_per_sample;
  g.mask_out_of_bounds = a.mask_out_of_bounds;
  g.contract_coords = a.contract_coords;
  return g;
}

int kplanes_render_backward_total_width(const LpKPlanesRenderArgs& a) {
  LpRendererArgs ra;
  decoder_view(a, a.grad_feature != nullptr, ra);
  GenPlan p;
  return make_plan(ra, p);
}

// `a` checked by lp_api.hip: n_rays > 0, n_samples >= 1, n_rays * n_samples < 2^31
int kplanes_render_launch(const LpKPlanesRenderArgs& a, bool backward, hipStream_t stream) {
  return backward ? backward_launch(a, stream) : forward_launch(a, stream);
}

const char* build_info_kplanes_render() {
  return "{\"forward\": \"one wavefront per ray, lanes = samples in chunks of 64: scalar plane bases, the time-axis cell of a per-ray "
         "timestamp once per ray, geometry tile in LDS, lanes = channels gather whole plane rows, the decoder on LDS column tiles sized "
         "per tile (fp32 FMA, no private array) and the compositing scan in one launch; fixed-order sums\", \"backward\": \"one "
         "wavefront per ray, chunks far to near from the saved per-chunk -log T: the same gather, decoder backward, d feat through LDS, "
         "run-merged whole-row fp32 atomics into the planes; encoding gradient stored per ray, no atomics\"}";
}

}  // namespace lp

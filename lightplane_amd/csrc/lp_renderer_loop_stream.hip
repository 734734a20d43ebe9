// lp_renderer_loop_stream.hip -- FORWARD of the deep two-block decoders (hidden width 64 / 64 grid channels with more than two
// layers in an MLP) on the layer-looped bf16x3 family: lp_renderer_forward_ws (include/lightplane_hip.h).
//
// The backward of these shapes runs the shape-generic kernels (their dW accumulators and kept activations exceed the register file,
// DESIGN.md 7), so lp_renderer_kernel_family() keeps reporting 0 for them.  The forward has no such limit: renderer_fwd_loop<C, 2, TG>
// already loops to 4 trunk + 3 hidden head layers in registers; only the RESIDENCY of the weight images stops it -- 3/3/3 x 64 is 26
// block images (166 KB), 4/4/4 x 64 is 38 (242 KB), the LDS holds 160 KB (KB = 1 024 bytes throughout; a block image is 6 528 bytes).
//   * images that fit the LDS without the backward's per-wave tiles: renderer_fwd_loop as it is (family 3);
//   * the others: renderer_fwd_stream below (family 4).  The images live pre-split in global memory (three bf16 limbs in exactly the
//     LDS layout, written once per call by loop_pack_images into the caller's workspace); a leading run of layers stays resident,
//     the rest passes through a RING of two LDS slots: while the eight waves compute streamed layer k out of one slot, direct
//     global -> LDS loads (global_load_lds_dwordx4, no register staging) fill the other with layer k + 1.  One workgroup barrier
//     per streamed layer and sample step: "my loads have landed" and "I am done reading the slot that is overwritten next" are the
//     same barrier.
// The ring is workgroup-synchronous, so nothing may let a wave leave the sample loop on its own: with early termination the waves
// vote through LDS once per sample step (one more barrier), a wave whose rays are done keeps serving the ring, and the workgroup
// leaves together.  The vote is taken per PAIR of waves = 64 consecutive rays = one wavefront of the shape-generic kernels: the
// generic backward reads ONE last-marched sample per 64 rays (its readfirstlane of the closing checkpoint pair), so the forward has to
// stop those 64 rays at the same sample -- exactly where the generic forward stops them.  (That is also why a deep decoder whose
// images are resident takes this kernel, without a ring, when early termination is on.)
#include "lp_renderer_loop.h"

namespace lp {

constexpr int STREAM_MAX = LOOP_MAX_T + 2 * LOOP_MAX_H;  // layers on the matrix cores
constexpr int STREAM_NW = 8;                              // waves per workgroup: one workgroup per CU, two waves per SIMD
constexpr size_t STREAM_LDS = 160 * 1024;

struct LoopStream {
  const char* ws;          // pre-split images of the streamed layers (loop_pack_images)
  int n_res;               // leading layers (order: trunk, opacity head, colour head) whose images are resident in LDS
  int n_s;                 // streamed layers (the rest)
  int ring, slot;          // byte offset of the ring in LDS, bytes per slot (two slots)
  int flags;               // byte offset of the termination votes: int [2 step parities][STREAM_NW]
  int vote;                // early termination is on
  int src[STREAM_MAX];     // per streamed layer: byte offset inside ws
  int bytes[STREAM_MAX];   // ... and bytes (multiple of 16)
};

// images of the streamed layers -> workspace; one workgroup per streamed layer
__global__ void __launch_bounds__(256) loop_pack_images(const float* P, const LoopParams lp, const LoopStream st) {
  const int gi = st.n_res + (int)blockIdx.x;
  const LoopLayer& L = gi < lp.n_t ? lp.t[gi] : (gi < lp.n_t + lp.n_o ? lp.o[gi - lp.n_t] : lp.c[gi - lp.n_t - lp.n_o]);
  loop_write_images(const_cast<char*>(st.ws) + st.src[blockIdx.x], P, L, (int)threadIdx.x);
}

// this wave's share of the copy of streamed layer j into ring slot `slot`: 16 bytes per lane and instruction, the LDS destination
// of a direct load is wave-uniform base + 16 * lane
LP_DEV void stream_issue(const LoopStream& st, char* ldsb, int j, int slot, int wave, int lane) {
  typedef __attribute__((address_space(1))) const void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;
  const int bytes = st.bytes[j];
  const char* src = st.ws + st.src[j];
  char* dst = ldsb + st.ring + slot * st.slot;
  for (int u0 = wave * 64; u0 * 16 < bytes; u0 += STREAM_NW * 64) {  // wave-uniform
    const int u = u0 + lane;
    if (u * 16 < bytes) __builtin_amdgcn_global_load_lds((gptr_t)(src + (size_t)u * 16), (lptr_t)(dst + u0 * 16), 16, 0, 0);
  }
}
// the direct loads count on vmcnt; data they wrote is ordered for a ds_read only behind the wait + a barrier the reader has passed
LP_DEV void stream_barrier() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <int C, bool TG, int GM>
__global__ void __launch_bounds__(64 * STREAM_NW, 2) renderer_fwd_stream(const LpRendererArgs a, const LoopParams lp, const LoopStream st) {
  constexpr int NB = 2;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  char* const ldsb = reinterpret_cast<char*>(lds);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int h = lane >> 5, r = lane & 31;
  if (st.n_s > 0) stream_issue(st, ldsb, 0, 0, wave, lane);
  loop_stage<NB>(a, lp, lds, st.n_res);
  stream_barrier();
  const float* const geo = lds + lp.inf - Lds::INF;
  volatile int* const votes = reinterpret_cast<volatile int*>(ldsb + st.flags);
  const int64_t ray_id = ((int64_t)blockIdx.x * STREAM_NW + wave) * RAYS_PER_WAVE + r;
  const bool valid = ray_id < a.rays.n_rays;
  const int64_t rid = valid ? ray_id : 0;
  const Ray ray = load_ray(a.rays, rid);
  float enc[NB][16];
  loop_load_encoding<NB>(a, rid, h, lp.hin, enc);
  const int s_tot = a.march.num_samples + a.march.num_samples_inf;
  const int n_ckpt = ckpt_count(a.march);
  const float delta0 = (a.march.num_samples > 1) ? (ray.far_t - ray.near_t) / (float)(a.march.num_samples - 1) : 1.0f;
  float nlt = 0.0f, nlt_lo = 0.0f, t_prev = 1.0f, len = 0.0f, depth_prev = 0.0f;
  int s_last = s_tot - 1;
  float facc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  Sample<C> nx;
  int rc = 0;            // streamed layers consumed so far: layer number rc sits in slot rc & 1
  bool marching = true;  // wave-uniform; false: the 64 rays of this wave's pair are terminated, the wave only serves the ring
  for (int s = 0; s < s_tot; ++s) {
    bool done = true;
    if (marching) {
      fetch_sample<C, GM, true>(a, geo, ray, s, h, nx);
      const float depth = nx.depth, occ = nx.occ;
      const int zo = opaque_zero();
      const char* lbase = reinterpret_cast<const char*>(lds) + zo;
      const float* sm = lds + zo;
      // one layer: resident images at their place, streamed ones in the ring -- the next streamed layer's loads are issued in front
      // of the products, the barrier behind them
      auto layer = [&](const LoopLayer& L0, int gi, const float (&in)[NB][16], float (&out)[NB][16]) {
        const bool streamed = gi >= st.n_res;  // workgroup-uniform
        LoopLayer L = L0;
        if (streamed) {
          const int j = gi - st.n_res;
          stream_issue(st, ldsb, (j + 1 == st.n_s) ? 0 : j + 1, (rc + 1) & 1, wave, lane);
          L.img = st.ring + (rc & 1) * st.slot;
        }
        loop_layer_fwd<NB>(lbase, sm, L, lane, in, out);
        if (streamed) {
          stream_barrier();
          ++rc;
        }
      };
      float cur[NB][16], ho[NB][16], hc[NB][16];
      loop_pad_input<C, NB, TG>(nx.x0, cur);
#pragma unroll
      for (int l = 0; l < LOOP_MAX_T; ++l) {
        if (!TG && l < lp.n_t) {
          float nxt[NB][16];
          layer(lp.t[l], l, cur, nxt);
          loop_copy<NB>(nxt, cur);
        }
      }
      float cin[NB][16];
      if (TG) {
        float xc0[C / 2];
        gather_list<C, false>(a.color_grid, a.march.mask_out_of_bounds != 0, ray, nx.x, nx.y, nx.z, h, xc0);
        loop_pad_input<C, NB, true>(xc0, cin);
      } else {
        loop_copy<NB>(cur, cin);
      }
#pragma unroll
      for (int b = 0; b < NB; ++b) {
#pragma unroll
        for (int q = 0; q < 16; ++q) cin[b][q] += enc[b][q];
      }
      loop_copy<NB>(cur, ho);
#pragma unroll
      for (int l = 0; l < LOOP_MAX_H; ++l) {
        if (l < lp.n_o) {
          float nxt[NB][16];
          layer(lp.o[l], lp.n_t + l, ho, nxt);
          loop_copy<NB>(nxt, ho);
        }
      }
      loop_copy<NB>(cin, hc);
#pragma unroll
      for (int l = 0; l < LOOP_MAX_H; ++l) {
        if (l < lp.n_c) {
          float nxt[NB][16];
          layer(lp.c[l], lp.n_t + lp.n_o + l, hc, nxt);
          loop_copy<NB>(nxt, hc);
        }
      }
      const Heads hd = loop_heads_forward<NB>(sm, lp, h, ho, hc);
      float raw = hd.raw_o;
      const float delta = (s == 0) ? delta0 : depth - depth_prev;
      depth_prev = depth;
      if (a.noise_sigma > 0.0f) raw = raw + sample_noise(rid, s, a.rays.n_rays, s_tot, a.noise_seed) * a.noise_sigma;
      const float opacity = a.gain * softplus_f(raw) * occ;
      nlt_add(nlt, nlt_lo, opacity * delta);
      if (a.neg_log_t_ckpt && valid && h == 0) {
        const int ck = ckpt_index(s, a.march);
        if (ck >= 0) *reinterpret_cast<float2*>(a.neg_log_t_ckpt + (ray_id * n_ckpt + ck) * 2) = make_float2(nlt, nlt_lo);
      }
      const float tr = __expf(-nlt);
      const float w = t_prev - tr;
      t_prev = tr;
      len = fmaf(w, depth, len);
#pragma unroll
      for (int c = 0; c < 4; ++c) facc[c] = fmaf(w, sigmoid_f(hd.raw_c[c]) * occ, facc[c]);
      done = __ballot(valid && nlt < a.stop_neg_log_t) == 0;
    } else {
      // this wave's 64-ray pair is terminated: keep the ring turning for the waves that still march
      for (int j = 0; j < st.n_s; ++j) {
        stream_issue(st, ldsb, (j + 1 == st.n_s) ? 0 : j + 1, (rc + 1) & 1, wave, lane);
        stream_barrier();
        ++rc;
      }
    }
    if (st.vote) {  // workgroup-uniform
      // votes of step s in the set s & 1: a wave rewrites a set two steps later, behind the barrier of the step between, which no wave
      // passes before it has read this one
      volatile int* const v = votes + (s & 1) * STREAM_NW;
      if (lane == 0) v[wave] = done ? 1 : 0;
      stream_barrier();
      int all = 1;
#pragma unroll
      for (int k = 0; k < STREAM_NW; ++k) all &= v[k];
      all = __builtin_amdgcn_readfirstlane(all);
      const int pair = __builtin_amdgcn_readfirstlane(v[wave] & v[wave ^ 1]);
      if (marching && pair) {  // the rule of the generic forward: all 64 rays of a wavefront are through
        s_last = s;
        marching = false;
      }
      if (all) break;
    }
  }
  if (valid && h == 0) {
    write_ray_outputs(a, ray_id, len, nlt, facc);
    if (a.neg_log_t_ckpt) *reinterpret_cast<float2*>(a.neg_log_t_ckpt + (ray_id * n_ckpt + n_ckpt - 1) * 2) = make_float2((float)s_last, nlt_lo);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
struct StreamPlan {
  LoopParams p;
  LoopStream st;
  size_t lds;        // dynamic LDS of renderer_fwd_stream
  int64_t ws_bytes;  // workspace: the streamed layers' images back to back, no header
};

// Resident prefix + ring: the first layers (trunk, opacity head, colour head -- the order they run in) stay resident as long as they
// fit beside a ring of two slots of the largest layer; images that fit as a whole need no ring (single grid-list).
static StreamPlan stream_plan(const LpRendererArgs& a) {
  StreamPlan sp = {};
  sp.p = renderer_loop_params(a);
  LoopParams& p = sp.p;
  LoopStream& st = sp.st;
  LoopLayer* L[STREAM_MAX];
  int n = 0;
  for (int l = 0; l < p.n_t; ++l) L[n++] = &p.t[l];
  for (int l = 0; l < p.n_o; ++l) L[n++] = &p.o[l];
  for (int l = 0; l < p.n_c; ++l) L[n++] = &p.c[l];
  int total = 0, slot = 0;
  for (int i = 0; i < n; ++i) {
    const int b = loop_layer_bytes(L[i]->rows_in, L[i]->cols);
    total += b;
    slot = b > slot ? b : slot;
  }
  const int small = p.img_end - total;  // the small block in front of the images
  const int vote_bytes = 2 * STREAM_NW * 4;
  st.vote = a.stop_neg_log_t > 0.0f;
  // (a two-grid decoder always gets the ring laid out: renderer_fwd_loop has no eight-wave form for it -- two gathers per sample --, so
  // 0/4/4 x 64, whose 20 block images would fit, would run resident at ONE wave per SIMD; here its last layer is streamed at two)
  const bool tg = a.color_grid.n_grids > 0;
  if (!tg && (size_t)p.img_end + vote_bytes <= STREAM_LDS) {
    st.n_res = n;
    st.flags = p.img_end;
    sp.lds = (size_t)p.img_end + vote_bytes;
    return sp;
  }
  const int avail = (int)STREAM_LDS - vote_bytes - small - 2 * slot;
  int off = small, i = 0;
  for (; i < n && off - small + loop_layer_bytes(L[i]->rows_in, L[i]->cols) <= avail; ++i) {
    L[i]->img = off;
    off += loop_layer_bytes(L[i]->rows_in, L[i]->cols);
  }
  st.n_res = i;
  st.n_s = n - i;
  st.ring = off;
  st.slot = slot;
  st.flags = off + 2 * slot;
  sp.lds = (size_t)st.flags + vote_bytes;
  for (int j = 0; i < n; ++i, ++j) {
    L[i]->img = st.ring;  // (set per use by the kernel)
    st.src[j] = (int)sp.ws_bytes;
    st.bytes[j] = loop_layer_bytes(L[i]->rows_in, L[i]->cols);
    sp.ws_bytes += st.bytes[j];
  }
  p.img_end = st.ring;
  return sp;
}

// The shapes of the new ground: what renderer_loop_supported() turns down ONLY for "hidden 64 / 64 grid channels with more than 2
// layers per MLP", default arithmetic.
bool renderer_deep_forward_supported(const LpRendererArgs& a) {
  const char* why = "";
  if (a.arithmetic != LP_ARITH_DEFAULT) return false;
  if (renderer_loop_supported(a, &why)) return false;  // (not new ground: lp_renderer_kernel_family answers)
  return renderer_loop_supported_forward(a, &why);
}

// 3: the images are resident (renderer_fwd_loop; with early termination renderer_fwd_stream without a ring), 4: streamed
int renderer_deep_forward_family(const LpRendererArgs& a) { return stream_plan(a).st.n_s > 0 ? 4 : 3; }
int64_t renderer_deep_forward_workspace(const LpRendererArgs& a) { return stream_plan(a).ws_bytes; }

template <int C, bool TG, int GM>
static int launch_stream(const LpRendererArgs& a, const StreamPlan& sp, hipStream_t stream) {
  int rc;
  if ((rc = loop_set_lds(renderer_fwd_stream<C, TG, GM>, sp.lds))) return rc;
  const unsigned nb = (unsigned)((a.rays.n_rays + STREAM_NW * RAYS_PER_WAVE - 1) / (STREAM_NW * RAYS_PER_WAVE));
  hipLaunchKernelGGL((renderer_fwd_stream<C, TG, GM>), dim3(nb), dim3(64 * STREAM_NW), sp.lds, stream, a, sp.p, sp.st);
  return LP_OK;
}

int renderer_forward_deep(const LpRendererArgs& a, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  StreamPlan sp = stream_plan(a);
  if (sp.st.n_s > 0 && (!workspace || workspace_bytes < sp.ws_bytes))
    return set_error(LP_EINVAL, "lp_renderer_forward_ws: this decoder streams its weight images and needs a workspace of %lld bytes "
                     "(lp_renderer_forward_workspace_bytes), got %s of %lld", (long long)sp.ws_bytes, workspace ? "one" : "NULL",
                     (long long)workspace_bytes);
  if (sp.st.n_s > 0 && ((uintptr_t)workspace & 15))
    return set_error(LP_EINVAL, "lp_renderer_forward_ws: the workspace has to be 16-byte aligned");
  if (a.rays.n_rays == 0) return LP_OK;
  // The backward of these shapes is the shape-generic one, which reports ONE segment, so normalized_renderer_args() has cleared
  // seg_prefix; renderer_fwd_stream writes no segment records, and the resident half below must not start to where this half cannot
  if (a.seg_prefix)
    return set_error(LP_EINVAL, "lp_renderer_forward_ws: seg_prefix is set, but the backward of a deep hidden-64 decoder has one segment");
  // resident images, no early termination: the family's forward as it is (forward-only LDS, eight-wave workgroups where it has them)
  if (sp.st.n_s == 0 && !sp.st.vote) return renderer_forward_loop(a, stream);
  if (sp.st.n_s > 0) {
    sp.st.ws = static_cast<const char*>(workspace);
    hipLaunchKernelGGL(loop_pack_images, dim3(sp.st.n_s), dim3(256), 0, stream, a.mlp_params, sp.p, sp.st);
  }
  const bool tg = a.color_grid.n_grids > 0, tri = is_canonical_triplane(a.grid);
  int rc;
  if (a.grid.channels == 64) rc = launch_stream<64, false, GM_GENERIC>(a, sp, stream);
  else if (a.grid.channels == 16) rc = tg ? launch_stream<16, true, GM_GENERIC>(a, sp, stream)
                                     : tri ? launch_stream<16, false, GM_TRIPLANE>(a, sp, stream) : launch_stream<16, false, GM_GENERIC>(a, sp, stream);
  else rc = tg ? launch_stream<32, true, GM_GENERIC>(a, sp, stream)
          : tri ? launch_stream<32, false, GM_TRIPLANE>(a, sp, stream) : launch_stream<32, false, GM_GENERIC>(a, sp, stream);
  if (rc) return rc;
  return check_launch("renderer_fwd_stream");
}

const char* build_info_loop_stream() {
  return "{\"kernel\": \"renderer_fwd_stream: layer-looped bf16x3 forward, resident prefix + two-slot LDS ring fed by "
         "global_load_lds_dwordx4, 8 waves per workgroup\", \"shapes\": \"hidden 64 / 64 grid channels, 3-4 layers in an MLP\"}";
}

}  // namespace lp

// lp_kplanes_scaffold.hip -- occupancy scaffold of a space-time plane field over a set of timestamps: the decoder's opacity on the
// regular lattice of a [B, D, H, W] scaffold, its maximum over the timestamps, thresholded and dilated (C ABI
// lp_kplanes_scaffold_*, include/lightplane_hip_kplanes_scaffold.h, which holds the definition).  No lattice point, feature or
// per-timestamp opacity ever reaches memory.
//
// On a lattice a factorised field is cheaper than at arbitrary points: along one row (b, z, y fixed, x runs) the yz, yt and zt values
// are the same for every point, xy and xz do not depend on the timestamp, and only xt depends on both x and t.
//
// kplanes_scaffold_lattice<P>: one wavefront = one workgroup = up to 64 consecutive x of ONE lattice row; a row of W > 64 takes
// ceil(W / 64) workgroups, a row of W < 64 (and the tail of any row) leaves lanes idle: they recompute the row's last point and store
// nothing.
//   row-uniform  ks_uniform, lanes = channels: lane l < S C / 4 owns the float4 slice 4 l of the feature vector, loads the four vertices
//                of its scale's plane (whole rows of 4 C bytes per scale) and leaves the bilinear value in an LDS vector [S C]: yz once
//                per workgroup, yt and zt once per timestamp.  No lane = point repeats these loads.
//   gather       ks_gather, lanes = channels as kpp_gather (lp_kplanes_tile.h): C / 4 consecutive lanes serve one point with a float4
//                of channels each, 256 / C points per pass.  A point's geometry is its x alone -- i_y, i_z, i_t are wave-uniform --, so
//                a gather lane forms (i_x, f_x) of the point it serves from the point's index in registers: there is no geometry tile
//                and no barrier for one.  Consecutive points read consecutive or equal plane rows (row = i_x + n i_v): a pass reads a
//                contiguous span of each plane.  All vertex loads of a pass (4 per plane) are issued before the first use.
//   product      the encoding's order, ((((xy xz) yz) xt) yt) zt, plane by plane with kp_fold per plane: the same folds and the same
//                sequence of products as kpp_gather, so the features are those of kplanes_eval_mlp_opacity_only on the same points.
//   static part  (xy xz) yz does not depend on the timestamp; it is formed again per timestamp from L2 all the same.  An LDS tile
//                [S C][64] that kept it would cost a workgroup or more per compute unit at S C >= 64 (DESIGN.md 4.29 has the
//                arithmetic); that choice is reasoned from the LDS budget, not measured.
//   decoder      lane = point on LDS column tiles (sc_dense, lp_column_mlp.h): weights through wave-uniform scalar loads, plain fp32
//                FMA chains, no private array.  The tiles are sized by content: `in` [max(S C, widest hidden layer)][64] holds the
//                features and then every second layer's output, `hid` [widest hidden layer][64] the others.
//   time loop    inside the kernel; the running maximum of gain * softplus(raw) stays in a register.  In the occupancy modes the loop
//                ends once every valid lane of the wave is above the threshold (one wave vote per timestamp): max is monotone, so the
//                occupancy is the same bits.
// The result leaves as the opacity lattice, as 0 / 1 floats or as occupancy bytes for the separable dilation of lp_scaffold.hip
// (scaffold_dilate_launch).  64-bit row offsets; plain vector stores; no atomics: bit-reproducible; no host synchronisation.
#include "lp_column_mlp.h"
#include "lp_kplanes_planes.h"

namespace lp {

enum { KS_RAW = 0, KS_OCC_FLOAT = 1, KS_OCC_BYTE = 2 };  // what the lattice kernel stores

struct KsArgs {
  LpKPlanesScaffoldArgs a;
  void* out;          // [B, D, H, W] floats (KS_RAW, KS_OCC_FLOAT) or bytes (KS_OCC_BYTE)
  int32_t mode;
  int32_t x_chunks;   // workgroups per lattice row: ceil(W / 64)
  int32_t in_rows;    // rows of the tile the features go to: max(S C, widest hidden layer)
  int32_t hid_rows;   // rows of the other activation tile: widest hidden layer
  int32_t lanes_log;  // log2(C / 4): lanes per point of the gather
};

// lanes = channels: the bilinear value of plane J -- whose two coordinates (qu, qv) are the same for the whole lattice row -- for every
// scale, into dst[S C].  Lane l < S C / 4 forms channels 4 l .. 4 l + 3.  `pb`: the planes of the row's batch element.
template <int J>
LP_DEV void ks_uniform(const LpKPlanesScaffoldArgs& a, const float* pb, float qu, float qv, int lane, float* dst) {
  const int C = a.channels;
  if (4 * lane >= a.n_scales * C) return;
  const int s = 4 * lane / C, c0 = 4 * lane - s * C;
  int n = 0, nv = 0;  // (the layout tables are read at wave-uniform indices only: a select per scale, no indexed copy of the arguments)
  int64_t offset = 0;
  for (int i = 0; i < a.n_scales; ++i) {
    n = i == s ? a.spatial[i] : n;
    nv = i == s ? (KP_V(J) == 3 ? a.temporal[i] : a.spatial[i]) : nv;
    offset = i == s ? a.offset[i][J] : offset;
  }
  const KpAxis u = kp_axis(qu, n), v = kp_axis(qv, nv);
  const float* v0 = pb + (offset + (int64_t)u.i + (int64_t)n * (int64_t)v.i) * C + c0;
  const float* v1 = v0 + (int64_t)n * C;
  float4 tap[4];
  tap[0] = kp_ld4(v0);
  tap[1] = kp_ld4(v0 + C);
  tap[2] = kp_ld4(v1);
  tap[3] = kp_ld4(v1 + C);
  const float gu = 1.0f - u.f, gv = 1.0f - v.f;
  *reinterpret_cast<float4*>(dst + 4 * lane) = kp_fold(tap, gu * gv, u.f * gv, gu * v.f, u.f * v.f);
}

// the four vertices of a plane over (x, v) at base vertex (i_x, i_v) for this lane's float4 of channels
LP_DEV void ks_taps(const float* pb, int64_t offset, int n, int ix, int iv, int64_t C, int c0, float4* tap) {
  const float* v0 = pb + (offset + (int64_t)ix + (int64_t)n * (int64_t)iv) * C + c0;
  const float* v1 = v0 + (int64_t)n * C;
  tap[0] = kp_ld4(v0);
  tap[1] = kp_ld4(v0 + C);
  tap[2] = kp_ld4(v1);
  tap[3] = kp_ld4(v1 + C);
}

LP_DEV float4 ks_value(const float4* tap, float fu, float fv) {
  const float gu = 1.0f - fu, gv = 1.0f - fv;
  return kp_fold(tap, gu * gv, fu * gv, gu * fv, fu * fv);
}

// lanes = channels, float4 slices: scale s of the workgroup's 64 points (x0 .. x0 + 63 of the row, clamped to W - 1) into
// dst[(s C + c) * 64 + point].  uni: the row-uniform values yz | yt | zt, [S C] each (yt and zt exist with six planes only).  Every
// lane calls this.
template <int P>
LP_DEV void ks_gather(const KsArgs& k, const float* pb, int s, int x0, float y, float z, float t, const float* uni, float* dst, int lane) {
  const LpKPlanesScaffoldArgs& a = k.a;
  const int64_t C = a.channels;
  const int SC = a.n_scales * a.channels;
  const int n = a.spatial[s];
  const int W = a.shape.W;
  const int per = 64 >> k.lanes_log;  // points per pass
  const int c0 = 4 * (lane & ((1 << k.lanes_log) - 1));
  const int f0 = s * (int)C + c0;  // this lane's first feature
  constexpr bool time = P == 6;
  const KpAxis ay = kp_axis(y, n), az = kp_axis(z, n);
  const KpAxis at = time ? kp_axis(t, a.temporal[s]) : KpAxis{0, 0.0f, false};
  const float4 yz = *reinterpret_cast<const float4*>(uni + f0);
  float4 yt = make_float4(1.0f, 1.0f, 1.0f, 1.0f), zt = yt;
  if (time) {
    yt = *reinterpret_cast<const float4*>(uni + SC + f0);
    zt = *reinterpret_cast<const float4*>(uni + 2 * SC + f0);
  }
  for (int pass = 0; pass < (1 << k.lanes_log); ++pass) {
    const int r = pass * per + (lane >> k.lanes_log);  // < 64
    const int ix = min(x0 + r, W - 1);
    const KpAxis ax = kp_axis(lin01(ix, W) * 2.0f - 1.0f, n);
    float4 txy[4], txz[4], txt[4];
    ks_taps(pb, a.offset[s][0], n, ax.i, ay.i, C, c0, txy);
    ks_taps(pb, a.offset[s][1], n, ax.i, az.i, C, c0, txz);
    if (time) ks_taps(pb, a.offset[s][3], n, ax.i, at.i, C, c0, txt);
    float* d = dst + f0 * SC_WAVE + r;
    float4 acc = kp_mul(kp_mul(ks_value(txy, ax.f, ay.f), ks_value(txz, ax.f, az.f)), yz);
    if (time) acc = kp_mul(kp_mul(kp_mul(acc, ks_value(txt, ax.f, at.f)), yt), zt);
    d[0] = acc.x;
    d[SC_WAVE] = acc.y;
    d[2 * SC_WAVE] = acc.z;
    d[3 * SC_WAVE] = acc.w;
  }
}

template <int P>
__global__ void __launch_bounds__(SC_WAVE) kplanes_scaffold_lattice(const KsArgs k) {
  // in [in_rows][64] | hid [hid_rows][64] | yz, yt, zt [S C] each
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const LpKPlanesScaffoldArgs& a = k.a;
  const int lane = threadIdx.x;
  const int W = a.shape.W, H = a.shape.H, D = a.shape.D;
  const int x0 = (int)(blockIdx.x % (unsigned)k.x_chunks) * SC_WAVE;
  const int64_t line = blockIdx.x / (unsigned)k.x_chunks;  // (b D + z) H + y
  const int iy = (int)(line % H);
  const int iz = (int)((line / H) % D);
  const int b = (int)(line / ((int64_t)H * D));
  const bool valid = x0 + lane < W;
  const float y = lin01(iy, H) * 2.0f - 1.0f;
  const float z = lin01(iz, D) * 2.0f - 1.0f;

  const int S = a.n_scales, SC = S * a.channels;
  float* tin = lds;
  float* thid = tin + k.in_rows * SC_WAVE;
  float* uni = thid + k.hid_rows * SC_WAVE;
  const float* pb = a.planes + (int64_t)b * a.rows * a.channels;

  ks_uniform<2>(a, pb, y, z, lane, uni);
  const int T = P == 6 ? a.n_times : 1;
  float best = -INFINITY;
  for (int it = 0; it < T; ++it) {
    float t = 0.0f;
    if (P == 6) {  // (the gather before is behind a barrier: nobody reads yt and zt any more)
      t = sc_const(a.times)[it];
      ks_uniform<4>(a, pb, y, t, lane, uni + SC);
      ks_uniform<5>(a, pb, z, t, lane, uni + 2 * SC);
    }
    __syncthreads();  // the row-uniform values are there; the decoder before has read its tiles
    for (int s = 0; s < S; ++s) ks_gather<P>(k, pb, s, x0, y, z, t, uni, tin, lane);
    __syncthreads();
    float* cur = tin + lane;
    float* nxt = thid + lane;
    if (a.trunk.n_layers == 0) {  // the opacity head reads ReLU(features)
      for (int c = 0; c < SC; ++c) cur[c * SC_WAVE] = fmaxf(cur[c * SC_WAVE], 0.0f);
    }
    for (int l = 0; l < a.trunk.n_layers; ++l) {
      sc_dense(sc_const(mlp_w(a.mlp_params, a.trunk, l)), sc_const(mlp_b(a.mlp_params, a.trunk, l)), a.trunk.dims[l], a.trunk.dims[l + 1],
               a.trunk.dims[l + 1], cur, nxt, true);
      float* sw = cur;
      cur = nxt;
      nxt = sw;
    }
    for (int l = 0; l < a.opacity.n_layers; ++l) {
      const bool last = l == a.opacity.n_layers - 1;
      sc_dense(sc_const(mlp_w(a.mlp_params, a.opacity, l)), sc_const(mlp_b(a.mlp_params, a.opacity, l)), a.opacity.dims[l],
               a.opacity.dims[l + 1], last ? 1 : a.opacity.dims[l + 1], cur, nxt, !last);
      float* sw = cur;
      cur = nxt;
      nxt = sw;
    }
    best = fmaxf(best, a.gain * softplus_f(cur[0]));
    // occupancy: every point of the wave is decided -- a later timestamp can only raise the maximum (wave-uniform exit)
    if (k.mode != KS_RAW && __all(!valid || best > a.threshold)) break;
  }
  if (!valid) return;
  const int64_t p = line * W + x0 + lane;
  if (k.mode == KS_RAW) static_cast<float*>(k.out)[p] = best;
  else if (k.mode == KS_OCC_FLOAT) static_cast<float*>(k.out)[p] = best > a.threshold ? 1.0f : 0.0f;
  else static_cast<uint8_t*>(k.out)[p] = best > a.threshold ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// host side (`a` checked by lp_api.hip)
// ---------------------------------------------------------------------------------------------------------------------------

// the layout, the planes and the timestamps as the layout check of lp_api.hip reads them (there are no points)
LpKPlanesArgs kplanes_scaffold_view(const LpKPlanesScaffoldArgs& a) {
  LpKPlanesArgs g = {};
  g.planes = a.planes;
  g.times = a.times;
  g.rows = a.rows;
  for (int s = 0; s < LP_KPLANES_MAX_SCALES; ++s) {
    for (int j = 0; j < LP_KPLANES_MAX_PLANES; ++j) g.offset[s][j] = a.offset[s][j];
    g.spatial[s] = a.spatial[s];
    g.temporal[s] = a.temporal[s];
  }
  g.batch = a.batch;
  g.channels = a.channels;
  g.n_scales = a.n_scales;
  g.n_planes = a.n_planes;
  return g;
}

int kplanes_scaffold_launch(const LpKPlanesScaffoldArgs& a, float* out, void* workspace, bool occupancy, hipStream_t stream) {
  KsArgs k;
  k.a = a;
  const int SC = a.n_scales * a.channels;
  int hid = 1;  // widest layer output
  const LpMlp* ms[2] = {&a.trunk, &a.opacity};
  for (const LpMlp* m : ms)
    for (int l = 1; l <= m->n_layers; ++l) hid = m->dims[l] > hid ? m->dims[l] : hid;
  k.in_rows = SC > hid ? SC : hid;
  k.hid_rows = hid;
  k.x_chunks = (a.shape.W + SC_WAVE - 1) / SC_WAVE;
  k.lanes_log = 0;
  while ((4 << k.lanes_log) < a.channels) ++k.lanes_log;
  const bool dilate = occupancy && a.dilate > 0;
  k.mode = !occupancy ? KS_RAW : (dilate ? KS_OCC_BYTE : KS_OCC_FLOAT);
  k.out = dilate ? workspace : (void*)out;
  const size_t lds = ((size_t)(k.in_rows + k.hid_rows) * SC_WAVE + 3 * SC) * sizeof(float);  // <= 67 KB (LP_MAX_WIDTH 128)
  unsigned blocks;  // B D H ceil(W / 64) <= B D H W < 2^31
  if (int rc = launch_blocks("lp_kplanes_scaffold", (int64_t)a.shape.B * a.shape.D * a.shape.H * k.x_chunks, 1, blocks)) return rc;
#define LP_LAUNCH_KS(P)                                                                                                                 \
  do {                                                                                                                                  \
    hipError_t e = hipFuncSetAttribute((const void*)kplanes_scaffold_lattice<P>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    if (e != hipSuccess) return set_error((int)e, "hipFuncSetAttribute: %s", hipGetErrorString(e));                                     \
    hipLaunchKernelGGL((kplanes_scaffold_lattice<P>), dim3(blocks), dim3(SC_WAVE), lds, stream, k);                                     \
  } while (0)
  if (a.n_planes == 3) LP_LAUNCH_KS(3);
  else LP_LAUNCH_KS(6);
#undef LP_LAUNCH_KS
  if (int rc = check_launch("kplanes_scaffold_lattice")) return rc;
  if (!dilate) return LP_OK;
  return scaffold_dilate_launch(static_cast<uint8_t*>(workspace), out, a.shape, a.dilate, stream);
}

const char* build_info_kplanes_scaffold() {
  return "{\"lattice\": \"one wave per 64 consecutive x of one lattice row; yz (per workgroup) and yt, zt (per timestamp) formed by "
         "lanes = channels into LDS vectors; xy, xz, xt gathered by lanes = channels (C / 4 lanes per point, float4 slices, geometry "
         "from the point's index in registers), product in the encoding's order; lane = point decodes with sc_dense on content-sized "
         "tiles; time loop in the kernel, running maximum in a register, wave-vote early exit in the occupancy modes; the static "
         "product is formed again per timestamp\", \"dilation\": \"lp_scaffold.hip\"}";
}

}  // namespace lp

/*
 * lightplane_hip_kplanes_render.h -- rendering a space-time plane field (K-Planes / HexPlane; without time planes the Hadamard
 * tri-plane) along rays at caller-given sample depths: encoding, decoder and compositing in one launch, forward and backward
 * (lp_kplanes_render.hip; an extension of lightplane_hip_kplanes_points.h, whose layout rules, encoding and decoder hold here, and of
 * lightplane_hip_hash_render.h, whose ray, sample and result fields and whose compositing hold here: plain C, fp32, contiguous tensors,
 * 16-byte aligned device pointers, asynchronous calls on `stream`).
 *
 *   ray_samples | importance_samples (depths, deltas) -> kplanes_render
 *
 * replaces the chain  ... -> lp_kplanes_points_forward -> lp_composite_forward: no points, opacity or colour tensor of size
 * [n_rays, n_samples] exists, neither in the forward nor in the backward.
 *
 * The family is declared here and not in one of the other headers so that their tables stay as they are.  lp_abi_sizeof(58) answers
 * for LpKPlanesRenderArgs; 56, 57 and 59 do not exist.
 */
#ifndef LIGHTPLANE_HIP_KPLANES_RENDER_H
#define LIGHTPLANE_HIP_KPLANES_RENDER_H

#include "lightplane_hip_kplanes_points.h"
#include "lightplane_hip_hash_render.h"

#ifdef __cplusplus
extern "C" {
#endif

/* With S = n_samples depths and deltas per ray (any values, any order), for sample s of ray r:
 *   p        = depths[r, s] * directions[r] + origins[r]            (formed in registers; contracted when contract_coords is set)
 *   opacity, colour[c < color_chn] = the decoder on the plane encoding of p at its timestamp (times[r], or times[r, s] with
 *              time_per_sample), exactly as LpKPlanesPointsArgs defines it (batch element clamp(grid_idx[r]), encoding[r] added to the
 *              colour head's input, gain, out-of-bounds mask, scaffold)
 *   od       = opacity * deltas[r, s],   N_s = sum_{j < s} od_j,   w_s = exp(-N_s) * (-expm1(-od_s))       (LpCompositeArgs)
 *   ray_length[r] = sum_s w_s depths[r, s],   neg_log_t[r] = N_S,   feature[r, c] = sum_s w_s colour_s[c],   weights[r, s] = w_s
 *
 * lp_kplanes_render_forward:  one wavefront per ray, lanes = samples, chunks of 64 samples with the -log T carried between them.  The
 *   batch element is uniform over the wave, so every plane's base row is a scalar; with one timestamp per ray the time-axis cell of
 *   every scale is formed once per ray.  Per chunk and scale lane = sample leaves the geometry in an LDS tile, lanes = channels gather
 *   whole plane rows into the decoder's first column tile (the gather of lp_kplanes_points_forward), lane = sample runs trunk and
 *   heads; then the scan of lp_composite_forward, and the sums leave in a fixed order: no atomics, every result is bit-reproducible.
 *   The LDS tiles are sized by what each holds (lp_kplanes_render.hip).  ray_length, neg_log_t, feature and weights are WRITTEN
 *   entirely where non-NULL (NULL = not stored).  feature == NULL: the colour head is not evaluated -- the colour MLP and the encoding
 *   are never read (color.n_layers may then be 0 and encoding NULL) and the other results are the same bit for bit.  chunk_nlt
 *   [n_rays, lp_render_samples_chunks(S)] is WRITTEN entirely where non-NULL: the -log T each chunk starts from, the only thing the
 *   backward reads that the forward wrote.
 * lp_kplanes_render_backward: a workgroup (one wavefront) takes a run of consecutive rays and walks each ray's chunks far -> near:
 *   the same gather, the decoder, T from chunk_nlt (required) and the scan inside the chunk, and with
 *     v_s = grad_ray_length depth_s + <grad_feature, colour_s> + grad_weights_s,   d od_s = T_{s+1} v_s - sum_{j > s} w_j v_j + grad_neg_log_t
 *     d raw_s = d od_s delta_s gain occ softplus'(raw_s),   d craw_s[c] = w_s grad_feature[c] occ sigmoid'(craw_s[c])
 *   back through the heads and the trunk to the features' gradient, which goes through LDS to lanes = channels.  grad_* upstreams:
 *   NULL = zeros (all four NULL: nothing is launched; grad_feature NULL: the colour head is not evaluated and its parameters get no
 *   contribution).  Results, each may be NULL (skipped): grad_planes [batch, rows, C] and grad_mlp_params [n_mlp_params] are
 *   ACCUMULATED with fp32 atomics into buffers the caller has zeroed (groups of C lanes walk consecutive samples of ONE ray and add a
 *   plane's four vertex sums, whole rows, only where that plane's base row changes; rows no sample touches stay exactly 0);
 *   grad_encoding [n_rays, encoding_dim] is WRITTEN entirely (a fixed-order sum, no atomics, bit-reproducible; zeros without
 *   grad_feature).  No derivative divides by a plane value.  depths, deltas, origins, directions and times get no gradient.
 * Any S >= 1 with n_rays * S < 2^31.  n_rays == 0 launches nothing.  No workspace, no allocation, no host synchronisation:
 * graph-capturable.  Row offsets are 64-bit.  Before anything touches the device: LP_ENULL for NULL args / planes / mlp_params and,
 * with n_rays > 0, origins / directions / grid_idx / depths / deltas, NULL times with n_planes == 6, a NULL encoding where the colour
 * head runs or (backward) a NULL chunk_nlt; LP_EINVAL for n_rays < 0, n_samples < 1, an under-aligned pointer (the message begins with
 * the field) and what LpKPlanesPointsArgs lists for the layout, the decoder and the scaffold; LP_EUNSUPPORTED for channels outside
 * {4, 8, 16, 32, 64}, S * C > LP_MAX_WIDTH, widths outside [1, LP_MAX_WIDTH], n_rays * n_samples >= 2^31 or (backward) layer widths
 * beyond 1024 in total. */
typedef struct LpKPlanesRenderArgs {
  const float* planes;                 /* [batch, rows, C] read */
  float* grad_planes;                  /* [batch, rows, C] accumulated into (backward), or NULL */
  const float* times;                  /* [n_rays] or [n_rays, S] read (n_planes == 6); NULL (n_planes == 3) */
  int64_t rows;                        /* rows per batch element */
  int64_t offset[LP_KPLANES_MAX_SCALES][LP_KPLANES_MAX_PLANES]; /* the layout: as in LpKPlanesArgs */
  int32_t spatial[LP_KPLANES_MAX_SCALES];
  int32_t temporal[LP_KPLANES_MAX_SCALES];
  int32_t batch;
  int32_t channels;                    /* C */
  int32_t n_scales;                    /* number of scales */
  int32_t n_planes;                    /* P: 3 or 6 */
  int32_t time_per_sample;             /* 0: times [n_rays]; 1: times [n_rays, S] */
  int32_t mask_out_of_bounds;
  int32_t contract_coords;
  int32_t color_chn;                   /* real colour channels (<= color.dims[last]) */
  const float* mlp_params;             /* the decoder's flat parameter vector: trunk | opacity | colour */
  int64_t n_mlp_params;
  LpMlp trunk, opacity, color;         /* as in LpKPlanesPointsArgs; the trunk (without one: the heads) reads n_scales * C inputs */
  float gain;
  int32_t encoding_dim;                /* == the colour head's input width */
  const float* scaffold;               /* NULL or [B, D, H, W] occupancy (0 / 1 floats) */
  LpGrid scaffold_shape;               /* B, D, H, W of the scaffold (row_offset and data ignored) */
  const float* origins;                /* [n_rays, 3] read */
  const float* directions;             /* [n_rays, 3] read */
  const int32_t* grid_idx;             /* [n_rays] read: batch element of each ray */
  const float* encoding;               /* [n_rays, encoding_dim] read */
  const float* depths;                 /* [n_rays, S] read */
  const float* deltas;                 /* [n_rays, S] read */
  int64_t n_rays;
  int32_t n_samples;                   /* S >= 1 */
  int32_t reserved;
  /* forward results (WRITTEN entirely; NULL = not stored) */
  float* ray_length;                   /* [n_rays] */
  float* neg_log_t;                    /* [n_rays] */
  float* feature;                      /* [n_rays, color_chn]; NULL = no colour head */
  float* weights;                      /* [n_rays, S] */
  float* chunk_nlt;                    /* [n_rays, lp_render_samples_chunks(S)]; forward: WRITTEN entirely, backward: read */
  /* backward: upstream gradients (NULL = zeros) */
  const float* grad_ray_length;        /* [n_rays] */
  const float* grad_neg_log_t;         /* [n_rays] */
  const float* grad_feature;           /* [n_rays, color_chn] */
  const float* grad_weights;           /* [n_rays, S] */
  /* backward results (NULL = skip; grad_planes above) */
  float* grad_mlp_params;              /* [n_mlp_params] (accumulated) */
  float* grad_encoding;                /* [n_rays, encoding_dim] WRITTEN entirely */
} LpKPlanesRenderArgs;
int lp_kplanes_render_forward(const LpKPlanesRenderArgs* args, void* stream);
int lp_kplanes_render_backward(const LpKPlanesRenderArgs* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LIGHTPLANE_HIP_KPLANES_RENDER_H */

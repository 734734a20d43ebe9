/*
 * lightplane_hip_hash_render.h -- rendering a multiresolution hash-grid field along rays at caller-given sample depths: encoding,
 * decoder and compositing in one launch, forward and backward (lp_hash_render.hip; an extension of lightplane_hip_hash_points.h, whose
 * layout rules, encoding and decoder hold here, and of lightplane_hip_render_samples.h, whose compositing holds here: plain C, fp32,
 * contiguous tensors, 16-byte aligned device pointers, asynchronous calls on `stream`).
 *
 *   ray_samples | importance_samples (depths, deltas) -> hash_render
 *
 * replaces the chain  ... -> lp_hash_points_forward -> lp_composite_forward: no points, opacity or colour tensor of size
 * [n_rays, n_samples] exists, neither in the forward nor in the backward.
 *
 * The family is declared here and not in one of the other headers so that their tables stay as they are.  lp_abi_sizeof(46) answers
 * for LpHashRenderArgs; 44, 45 and 47 do not exist.
 */
#ifndef LIGHTPLANE_HIP_HASH_RENDER_H
#define LIGHTPLANE_HIP_HASH_RENDER_H

#include "lightplane_hip_hash_points.h"
#include "lightplane_hip_render_samples.h"

#ifdef __cplusplus
extern "C" {
#endif

/* With S = n_samples depths and deltas per ray (any values, any order; runs of equal depths and zero deltas included), for sample s
 * of ray r:
 *   p        = depths[r, s] * directions[r] + origins[r]            (formed in registers; contracted when contract_coords is set)
 *   opacity, colour[c < color_chn] = the decoder on the hash-grid encoding of p, exactly as LpHashPointsArgs defines it (batch element
 *              clamp(grid_idx[r]), encoding[r] added to the colour head's input, gain, out-of-bounds mask, scaffold)
 *   od       = opacity * deltas[r, s],   N_s = sum_{j < s} od_j,   w_s = exp(-N_s) * (-expm1(-od_s))       (LpCompositeArgs)
 *   ray_length[r] = sum_s w_s depths[r, s],   neg_log_t[r] = N_S,   feature[r, c] = sum_s w_s colour_s[c],   weights[r, s] = w_s
 * There is no opacity noise and no early termination; the opacity is not clamped.
 *
 * lp_hash_render_forward:  one wavefront per ray, lanes = samples, chunks of 64 samples with the -log T carried between them.  The
 *   batch element is uniform over the wave, so every level's table base is a scalar and a lane carries only its entry offsets; the
 *   decoder is the body of lp_hash_points_forward, the scan that of lp_composite_forward, and the sums leave in a fixed order: no
 *   atomics, every result is bit-reproducible.  ray_length, neg_log_t, feature and weights are WRITTEN entirely where non-NULL (NULL =
 *   that result is not stored).  feature == NULL: the colour head is not evaluated -- the colour MLP and the encoding are never read
 *   (color.n_layers may then be 0 and encoding NULL) and the other results are the same bit for bit.  chunk_nlt
 *   [n_rays, lp_render_samples_chunks(S)] is WRITTEN entirely where non-NULL: the -log T each chunk starts from, the only thing the
 *   backward reads that the forward wrote.
 * lp_hash_render_backward: one wavefront per ray, chunks far -> near, a workgroup takes a run of consecutive rays.  The lane recomputes
 *   its sample's features and decoder, T comes from chunk_nlt (required) and the scan inside the chunk, and with
 *     v_s = grad_ray_length depth_s + <grad_feature, colour_s> + grad_weights_s,   d od_s = T_{s+1} v_s - sum_{j > s} w_j v_j + grad_neg_log_t
 *   the decoder's upstream gradients are formed in registers:
 *     d raw_s = d od_s delta_s gain occ softplus'(raw_s),   d craw_s[c] = w_s grad_feature[c] occ sigmoid'(craw_s[c])
 *   and go back through the heads and the trunk to the features' gradient.  grad_* upstreams: NULL = zeros (all four NULL: nothing is
 *   launched; grad_feature NULL: the colour head is not evaluated and its parameters get no contribution).  Results, each may be NULL
 *   (skipped): grad_table [batch, entries, F] and grad_mlp_params [n_mlp_params] are ACCUMULATED with fp32 atomics into buffers the
 *   caller has zeroed (consecutive lanes are consecutive samples of ONE ray: those that share a level's cell form a run whose first
 *   lane adds the run's sum); grad_encoding [n_rays, encoding_dim] is WRITTEN entirely (a fixed-order sum, no atomics,
 *   bit-reproducible; zeros without grad_feature).  depths, deltas, origins and directions get no gradient.
 * Any S >= 1 with n_rays * S < 2^31.  n_rays == 0 launches nothing.  No workspace, no allocation, no host synchronisation:
 * graph-capturable.  Before anything touches the device: LP_ENULL for NULL args / table / origins / directions / grid_idx / depths /
 * deltas / mlp_params, a NULL encoding where the colour head runs or (backward) a NULL chunk_nlt; LP_EINVAL for n_rays < 0,
 * n_samples < 1, an under-aligned pointer (the message begins with the field) and what LpHashPointsArgs lists for the layout, the
 * decoder and the scaffold; LP_EUNSUPPORTED for features_per_level outside {1, 2, 4, 8}, n_levels * F > LP_MAX_WIDTH, widths outside
 * [1, LP_MAX_WIDTH], n_rays * n_samples >= 2^31 or (backward) layer widths beyond 1024 in total. */
typedef struct LpHashRenderArgs {
  const float* table;                  /* [batch, entries, F] read */
  float* grad_table;                   /* [batch, entries, F] accumulated into (backward), or NULL */
  int64_t entries;                     /* E: entries per batch element */
  int64_t offset[LP_HASH_MAX_LEVELS];  /* the layout: as in LpHashGridArgs */
  int32_t resolution[LP_HASH_MAX_LEVELS];
  int32_t size[LP_HASH_MAX_LEVELS];
  int32_t hashed[LP_HASH_MAX_LEVELS];
  int32_t batch;
  int32_t features_per_level;          /* F */
  int32_t n_levels;                    /* L */
  int32_t mask_out_of_bounds;
  int32_t contract_coords;
  int32_t color_chn;                   /* real colour channels (<= color.dims[last]) */
  const float* mlp_params;             /* the decoder's flat parameter vector: trunk | opacity | colour */
  int64_t n_mlp_params;
  LpMlp trunk, opacity, color;         /* as in LpHashPointsArgs; the trunk (without one: the heads) reads L * F inputs */
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
  /* backward results (NULL = skip; grad_table above) */
  float* grad_mlp_params;              /* [n_mlp_params] (accumulated) */
  float* grad_encoding;                /* [n_rays, encoding_dim] WRITTEN entirely */
} LpHashRenderArgs;
int lp_hash_render_forward(const LpHashRenderArgs* args, void* stream);
int lp_hash_render_backward(const LpHashRenderArgs* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LIGHTPLANE_HIP_HASH_RENDER_H */

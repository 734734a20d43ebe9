/*
 * lightplane_hip_render_samples.h -- rendering at caller-given sample depths: the decoder and the compositing of the march in pieces
 * in one launch (lp_render_samples.hip; an extension of lightplane_hip.h, whose Conventions hold here: plain C, fp32, contiguous
 * tensors, 16-byte aligned device pointers, asynchronous calls on `stream`).
 *
 *   ray_samples | importance_samples (depths, deltas) -> render_samples
 *
 * replaces the chain  ... -> lp_points_forward -> lp_composite_forward  where the decoder is the library's own: no points, opacity
 * or colour tensor of size [n_rays, n_samples] exists, neither in the forward nor in the backward.
 *
 * The family is declared here and not in one of the other headers so that their tables stay as they are.  lp_abi_sizeof(30) answers
 * for LpRenderSamplesArgs; 27, 28, 29 and 31 do not exist.
 */
#ifndef LIGHTPLANE_HIP_RENDER_SAMPLES_H
#define LIGHTPLANE_HIP_RENDER_SAMPLES_H

#include "lightplane_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* With S = n_samples depths and deltas per ray (any values, any order: the fine pass of a coarse-to-fine march hands in the sorted
 * result of lp_importance_samples_forward, runs of equal depths and zero deltas included), for sample s of ray r:
 *   p        = depths[r, s] * directions[r] + origins[r]            (formed in registers; contracted when contract_coords is set)
 *   opacity, colour[c < color_chn] = the decoder at p, exactly as LpPointsArgs defines it (grid-list, colour grid-list, trunk / heads,
 *              encoding[r] added to the colour head's input, gain, out-of-bounds mask, scaffold)
 *   od       = opacity * deltas[r, s],   N_s = sum_{j < s} od_j,   w_s = exp(-N_s) * (-expm1(-od_s))       (LpCompositeArgs)
 *   ray_length[r] = sum_s w_s depths[r, s],   neg_log_t[r] = N_S,   feature[r, c] = sum_s w_s colour_s[c],   weights[r, s] = w_s
 * There is no opacity noise and no early termination; the opacity is not clamped.
 *
 * lp_render_samples_forward:  one wavefront per ray, lanes = samples, chunks of 64 samples with the -log T carried between them.  The
 *   lane decodes its sample with the body of lp_points_forward (activations in LDS column tiles, fp32 FMA chains, no scratch), the
 *   wave scans od, and the sums leave in a fixed order: every result is bit-reproducible.  ray_length, neg_log_t, feature and weights
 *   are WRITTEN entirely where non-NULL (NULL = that result is not stored).  chunk_nlt [n_rays, lp_render_samples_chunks(S)] is
 *   WRITTEN entirely where non-NULL: the -log T each chunk starts from, the only thing the backward reads that the forward wrote.
 * lp_render_samples_backward: one wavefront per ray, chunks far -> near, a workgroup takes a run of consecutive rays.  The lane
 *   recomputes its sample's decoder (the recompute of lp_points_backward: wide layers on the fp32 matrix cores), T comes from
 *   chunk_nlt (required) and the scan inside the chunk, and with
 *     v_s = grad_ray_length depth_s + <grad_feature, colour_s> + grad_weights_s,   d od_s = T_{s+1} v_s - sum_{j > s} w_j v_j + grad_neg_log_t
 *   the decoder's upstream gradients are formed in registers:
 *     d raw_s = d od_s delta_s gain occ softplus'(raw_s),   d craw_s[c] = w_s grad_feature[c] occ sigmoid'(craw_s[c])
 *   and go back through the heads, the trunk and the gather as in lp_points_backward.  grad_* upstreams: NULL = zeros (all four NULL:
 *   nothing is launched; grad_feature NULL: the colour head is not evaluated).  Results, each may be NULL (skipped):
 *   grad_grid / grad_grid_list, grad_color_grid / grad_color_grid_list and grad_mlp_params [n_mlp_params] are ACCUMULATED with atomics
 *   into buffers the caller has zeroed; grad_encoding [n_rays, encoding_dim] is WRITTEN entirely (a ray is one wavefront's: a fixed
 *   order sum, no atomics, bit-reproducible).  depths, deltas, origins and directions get no gradient.
 * Any S >= 1 with n_rays * S < 2^31; any layer counts, widths and channels up to LP_MAX_WIDTH (backward: layer widths summing to at
 * most 1024, as lp_points_backward).  n_rays == 0 launches nothing.  No allocation, no host synchronisation: graph-capturable.
 * Before anything touches the device: LP_ENULL for NULL args / origins / directions / grid_idx / encoding / depths / deltas /
 * mlp_params, a grid without data or (backward) a NULL chunk_nlt; LP_EINVAL for n_rays < 0, n_samples < 1, an under-aligned pointer
 * (the message begins with the field) and what LpPointsArgs lists for the decoder, the grid-lists and the scaffold; LP_EUNSUPPORTED
 * for n_rays * n_samples >= 2^31, widths or channels outside [1, LP_MAX_WIDTH] or (backward) layer widths beyond 1024 in total. */
typedef struct LpRenderSamplesArgs {
  LpGridList grid;             /* feature grid-list */
  LpGridList color_grid;       /* n_grids == 0: single grid-list (trunk MLP used) */
  const float* mlp_params;     /* the decoder's flat parameter vector: trunk | opacity | colour */
  int64_t n_mlp_params;
  LpMlp trunk, opacity, color; /* as in LpRendererArgs */
  int32_t color_chn;           /* real colour channels (<= color.dims[last]) */
  float gain;
  int32_t mask_out_of_bounds;
  int32_t contract_coords;
  const float* origins;        /* [n_rays, 3] read */
  const float* directions;     /* [n_rays, 3] read */
  const int32_t* grid_idx;     /* [n_rays] read: batch element of each ray, as LpRays.grid_idx */
  const float* encoding;       /* [n_rays, encoding_dim] read */
  int32_t encoding_dim;        /* == the colour head's input width */
  int32_t n_samples;           /* S >= 1 */
  int64_t n_rays;
  const float* depths;         /* [n_rays, S] read */
  const float* deltas;         /* [n_rays, S] read */
  const float* scaffold;       /* NULL or [B, D, H, W] occupancy (0 / 1 floats) */
  LpGrid scaffold_shape;       /* B, D, H, W of the scaffold (row_offset and data ignored) */
  /* forward results (WRITTEN entirely; NULL = not stored) */
  float* ray_length;           /* [n_rays] */
  float* neg_log_t;            /* [n_rays] */
  float* feature;              /* [n_rays, color_chn] */
  float* weights;              /* [n_rays, S] */
  float* chunk_nlt;            /* [n_rays, lp_render_samples_chunks(S)]; forward: WRITTEN entirely, backward: read */
  /* backward: upstream gradients (NULL = zeros) */
  const float* grad_ray_length; /* [n_rays] */
  const float* grad_neg_log_t;  /* [n_rays] */
  const float* grad_feature;    /* [n_rays, color_chn] */
  const float* grad_weights;    /* [n_rays, S] */
  /* backward results (NULL = skip) */
  float* grad_grid;            /* like grid.data (accumulated) */
  float* grad_color_grid;      /* like color_grid.data (accumulated) */
  float* grad_grid_list[LP_MAX_GRIDS];        /* per-grid buffers, as in LpRendererArgs (accumulated) */
  float* grad_color_grid_list[LP_MAX_GRIDS];
  float* grad_mlp_params;      /* [n_mlp_params] (accumulated) */
  float* grad_encoding;        /* [n_rays, encoding_dim] WRITTEN entirely */
} LpRenderSamplesArgs;
int lp_render_samples_forward(const LpRenderSamplesArgs* args, void* stream);
int lp_render_samples_backward(const LpRenderSamplesArgs* args, void* stream);
/* floats per ray of chunk_nlt: ceil(n_samples / 64); 0 for n_samples < 1 */
int lp_render_samples_chunks(int32_t n_samples);

#ifdef __cplusplus
}
#endif

#endif /* LIGHTPLANE_HIP_RENDER_SAMPLES_H */

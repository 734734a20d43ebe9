/*
 * lightplane_hip_hash_points.h -- the decoder on a multiresolution hash grid at 3-D points, encoding and decoder in one launch, forward
 * and backward (lp_hash_points.hip; an extension of lightplane_hip_hash_grid.h, whose layout rules and encoding hold here, and of
 * lightplane_hip.h, whose Conventions and decoder hold here: plain C, fp32, contiguous tensors, 16-byte aligned device pointers,
 * asynchronous calls on `stream`).
 *
 *   feat[0 .. L F)  = the hash-grid encoding of point p = points[r, n]   (lp_hash_grid_forward: batch element clamp(grid_idx[r]), the
 *                     contraction when asked, all zero outside [-1, 1]^3 with mask_out_of_bounds)
 *   t = ReLU(trunk MLP(feat)) (ReLU(feat) without trunk layers),  raw = opacity MLP(t),  craw = colour MLP(t + encoding[r])
 *   opacity_out[r, n] = gain * softplus(raw) * occ,   color_out[r, n, c] = sigmoid(craw[c]) * occ, c < color_chn
 *   occ = 1, or with a scaffold its nearest-neighbour value at q (0 outside [-1, 1]^3), as in LpPointsArgs.
 *
 * The features never reach memory.  The family is declared here and not in one of the other headers so that their tables stay as
 * they are.  lp_abi_sizeof(42) answers for LpHashPointsArgs; 40, 41 and 43 do not exist.
 */
#ifndef LIGHTPLANE_HIP_HASH_POINTS_H
#define LIGHTPLANE_HIP_HASH_POINTS_H

#include "lightplane_hip_hash_grid.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lp_hash_points_forward: one lane per point, one wavefront per workgroup of 64 consecutive points.  The lane loops over the levels
 *   (8 corner loads issued before their first use) and writes the features into an LDS column tile; trunk and heads as
 *   lp_points_forward.  color_out == NULL: opacity only -- the colour MLP and the encoding are never read (color.n_layers may then be
 *   0 and encoding NULL).  No atomics: bit-reproducible.  The grad_* fields are ignored.
 * lp_hash_points_backward: recomputes features and decoder of every point (it reads nothing the forward wrote), forms
 *   d raw = grad_opacity * gain * occ * softplus'(raw) and d craw[c] = grad_color[c] * occ * sigmoid'(craw[c]) and goes back through
 *   the heads and the trunk to d feat.  grad_opacity / grad_color: NULL = zeros; both NULL: nothing is launched; with grad_color == NULL
 *   the colour head is not evaluated (its parameters get no contribution).  Every result pointer may be NULL (that gradient is
 *   skipped).  ACCUMULATED with fp32 atomics into buffers the caller has zeroed: grad_table [batch, entries, F] (consecutive lanes that
 *   share (b, cell) of a level form a run whose first lane adds the run's sum, as lp_hash_grid_backward_table), grad_mlp_params
 *   [n_mlp_params], grad_encoding [n_rays, encoding_dim].  WRITTEN: grad_points [n_rays, n_pts, 3], as lp_hash_grid_backward_points
 *   (0 on a clamped axis, through the contraction's Jacobian); bit-reproducible.  Nothing flows to grid_idx or the scaffold.
 * No workspace, no allocation, no host synchronisation: graph-capturable.  Entry offsets are 64-bit.
 * Before anything touches the device: LP_ENULL for NULL args / table / points / grid_idx / mlp_params / opacity_out (forward) or a
 * NULL encoding where the colour head runs; LP_EINVAL for an under-aligned pointer (the message begins with the field), a layout that
 * breaks a rule of lightplane_hip_hash_grid.h, MLPs that do not chain from L * F inputs or do not fit n_mlp_params, encoding_dim !=
 * the colour head's input width, color_chn outside the colour head's output, a scaffold of another batch size or an extent < 1;
 * LP_EUNSUPPORTED for features_per_level outside {1, 2, 4, 8}, n_levels * F > LP_MAX_WIDTH, widths outside [1, LP_MAX_WIDTH],
 * n_rays * n_pts >= 2^31 or (backward) layer widths beyond 1024 in total.  The checks are made whatever n_rays and n_pts are;
 * n_rays * n_pts == 0 then returns LP_OK without a launch. */
typedef struct LpHashPointsArgs {
  const float* table;                  /* [batch, entries, F] read */
  float* grad_table;                   /* [batch, entries, F] accumulated into (backward), or NULL */
  const float* points;                 /* [n_rays, n_pts, 3] read */
  const int32_t* grid_idx;             /* [n_rays] read: batch element of each row of points */
  int64_t entries;                     /* E: entries per batch element */
  int64_t n_rays;
  int64_t n_pts;
  int64_t offset[LP_HASH_MAX_LEVELS];     /* the layout: as in LpHashGridArgs */
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
  LpMlp trunk, opacity, color;         /* as in LpPointsArgs; the trunk (without one: the heads) reads L * F inputs */
  const float* encoding;               /* [n_rays, encoding_dim] */
  int32_t encoding_dim;                /* == the colour head's input width */
  float gain;
  const float* scaffold;               /* NULL or [B, D, H, W] occupancy (0 / 1 floats) */
  LpGrid scaffold_shape;               /* B, D, H, W of the scaffold (row_offset and data ignored) */
  /* forward results (written) */
  float* opacity_out;                  /* [n_rays, n_pts] */
  float* color_out;                    /* [n_rays, n_pts, color_chn]; NULL = opacity only */
  /* backward: upstream gradients (NULL = zeros) */
  const float* grad_opacity;           /* [n_rays, n_pts] */
  const float* grad_color;             /* [n_rays, n_pts, color_chn] */
  /* backward results (NULL = skip; grad_table above) */
  float* grad_mlp_params;              /* [n_mlp_params] (accumulated) */
  float* grad_encoding;                /* [n_rays, encoding_dim] (accumulated) */
  float* grad_points;                  /* [n_rays, n_pts, 3] (written) */
} LpHashPointsArgs;
int lp_hash_points_forward(const LpHashPointsArgs* args, void* stream);
int lp_hash_points_backward(const LpHashPointsArgs* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LIGHTPLANE_HIP_HASH_POINTS_H */

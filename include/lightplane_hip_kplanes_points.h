/*
 * lightplane_hip_kplanes_points.h -- the decoder on a space-time plane field (K-Planes / HexPlane; without time planes the Hadamard
 * tri-plane) at 3-D points, encoding and decoder in one launch, forward and backward (lp_kplanes_points.hip; an extension of
 * lightplane_hip_kplanes.h, whose layout rules and encoding hold here, and of lightplane_hip_hash_points.h, whose decoder holds here:
 * plain C, fp32, contiguous tensors, 16-byte aligned device pointers, asynchronous calls on `stream`).
 *
 *   feat[0 .. S C)  = the plane encoding of point p = points[r, n] at its timestamp   (lp_kplanes_forward: batch element
 *                     clamp(grid_idx[r]), the contraction when asked, all zero outside [-1, 1]^3 with mask_out_of_bounds)
 *   t = ReLU(trunk MLP(feat)) (ReLU(feat) without trunk layers),  raw = opacity MLP(t),  craw = colour MLP(t + encoding[r])
 *   opacity_out[r, n] = gain * softplus(raw) * occ,   color_out[r, n, c] = sigmoid(craw[c]) * occ, c < color_chn
 *   occ = 1, or with a scaffold its nearest-neighbour value at q (0 outside [-1, 1]^3), as in LpPointsArgs.
 *
 * The features never reach memory, and neither does their gradient.  The family is declared here and not in one of the other headers
 * so that their tables stay as they are.  lp_abi_sizeof(54) answers for LpKPlanesPointsArgs; 52, 53 and 55 do not exist.
 */
#ifndef LIGHTPLANE_HIP_KPLANES_POINTS_H
#define LIGHTPLANE_HIP_KPLANES_POINTS_H

#include "lightplane_hip_kplanes.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lp_kplanes_points_forward: one wavefront per workgroup of 64 consecutive points, in three phases.  Lane = point forms the geometry
 *   (per scale and plane the base row and the two fractions, into an LDS tile) and looks the scaffold up; lanes = channels load whole
 *   rows of 4 C bytes (the 4 P vertex loads of a point and scale issued before their first use), fold them into the P bilinear values,
 *   multiply those and write the product into the decoder's first LDS column tile; lane = point runs trunk and heads as
 *   lp_hash_points_forward.  color_out == NULL: opacity only -- the colour MLP and the encoding are never read (color.n_layers may
 *   then be 0 and encoding NULL).  No atomics: bit-reproducible.  The grad_* fields are ignored.
 * lp_kplanes_points_backward: recomputes features and decoder of every point (it reads nothing the forward wrote), forms
 *   d raw = grad_opacity * gain * occ * softplus'(raw) and d craw[c] = grad_color[c] * occ * sigmoid'(craw[c]) and goes back through
 *   the heads and the trunk to d feat, which goes through LDS to lanes = channels.  grad_opacity / grad_color: NULL = zeros; both NULL:
 *   nothing is launched; with grad_color == NULL the colour head is not evaluated (its parameters get no contribution).  Every result
 *   pointer may be NULL (that gradient is skipped).  ACCUMULATED with fp32 atomics into buffers the caller has zeroed: grad_planes
 *   [batch, rows, C] (groups of C lanes walk consecutive points and add a plane's four vertex sums, whole rows, only where that
 *   plane's base row changes, as lp_kplanes_backward_planes), grad_mlp_params [n_mlp_params], grad_encoding [n_rays, encoding_dim].
 *   WRITTEN: grad_points [n_rays, n_pts, 3] (0 on a clamped axis, through the contraction's Jacobian), formed in the same walk in a
 *   fixed order: bit-reproducible, and the same bits whichever other gradients are asked for.  No derivative divides by a plane
 *   value.  Nothing flows to times, grid_idx or the scaffold.
 * No workspace, no allocation, no host synchronisation: graph-capturable.  Row offsets are 64-bit.
 * Before anything touches the device: LP_ENULL for NULL args / planes / points / grid_idx / mlp_params / opacity_out (forward), NULL
 * times with n_planes == 6, or a NULL encoding where the colour head runs; LP_EINVAL for an under-aligned pointer (the message begins
 * with the field), a layout that breaks a rule of lightplane_hip_kplanes.h, MLPs that do not chain from S * C inputs or do not fit
 * n_mlp_params, encoding_dim != the colour head's input width, color_chn outside the colour head's output, a scaffold of another
 * batch size or an extent < 1; LP_EUNSUPPORTED for channels outside {4, 8, 16, 32, 64}, S * C > LP_MAX_WIDTH, widths outside
 * [1, LP_MAX_WIDTH], n_rays * n_pts >= 2^31 or (backward) layer widths beyond 1024 in total.  The checks are made whatever n_rays
 * and n_pts are; n_rays * n_pts == 0 then returns LP_OK without a launch. */
typedef struct LpKPlanesPointsArgs {
  const float* planes;                 /* [batch, rows, C] read */
  float* grad_planes;                  /* [batch, rows, C] accumulated into (backward), or NULL */
  const float* points;                 /* [n_rays, n_pts, 3] read */
  const float* times;                  /* [n_rays] or [n_rays, n_pts] read (n_planes == 6); NULL (n_planes == 3) */
  const int32_t* grid_idx;             /* [n_rays] read: batch element of each row of points */
  int64_t rows;                        /* rows per batch element */
  int64_t n_rays;
  int64_t n_pts;
  int64_t offset[LP_KPLANES_MAX_SCALES][LP_KPLANES_MAX_PLANES]; /* the layout: as in LpKPlanesArgs */
  int32_t spatial[LP_KPLANES_MAX_SCALES];
  int32_t temporal[LP_KPLANES_MAX_SCALES];
  int32_t batch;
  int32_t channels;                    /* C */
  int32_t n_scales;                    /* S */
  int32_t n_planes;                    /* P: 3 or 6 */
  int32_t time_per_point;              /* 0: times [n_rays]; 1: times [n_rays, n_pts] */
  int32_t mask_out_of_bounds;
  int32_t contract_coords;
  int32_t color_chn;                   /* real colour channels (<= color.dims[last]) */
  const float* mlp_params;             /* the decoder's flat parameter vector: trunk | opacity | colour */
  int64_t n_mlp_params;
  LpMlp trunk, opacity, color;         /* as in LpPointsArgs; the trunk (without one: the heads) reads S * C inputs */
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
  /* backward results (NULL = skip; grad_planes above) */
  float* grad_mlp_params;              /* [n_mlp_params] (accumulated) */
  float* grad_encoding;                /* [n_rays, encoding_dim] (accumulated) */
  float* grad_points;                  /* [n_rays, n_pts, 3] (written) */
} LpKPlanesPointsArgs;
int lp_kplanes_points_forward(const LpKPlanesPointsArgs* args, void* stream);
int lp_kplanes_points_backward(const LpKPlanesPointsArgs* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LIGHTPLANE_HIP_KPLANES_POINTS_H */

/*
 * lightplane_hip_ray_grid.h -- weighted splat and gather of a grid-list along rays at caller-given sample depths, without a decoder
 * (lp_ray_grid.hip; an extension of lightplane_hip.h, whose Conventions hold here: plain C, fp32, contiguous tensors, 16-byte aligned
 * device pointers, asynchronous calls on `stream`).
 *
 *   grid += weights[r, s] * features[r]   at   origins[r] + depths[r, s] * directions[r]        (lift a pixel feature by a depth distribution)
 *   out[r] = sum_s weights[r, s] * sample(grid, that point)                                     (render a feature grid with given weights)
 *
 * replaces  lp_point_splat / lp_point_gather  on an expanded [n_rays, n_samples, C] tensor: no tensor of that size exists, and the
 * per-ray vector is read once per ray.
 *
 * The family is declared here and not in one of the other headers so that their tables stay as they are.  lp_abi_sizeof(34) answers
 * for LpRayGridArgs; 31, 32, 33 and 35 do not exist.
 */
#ifndef LIGHTPLANE_HIP_RAY_GRID_H
#define LIGHTPLANE_HIP_RAY_GRID_H

#include "lightplane_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* With S = n_samples depths and weights per ray (any values, any order), the grid-list G (C channels), a per-ray vector F [n_rays, C],
 *   p_rs = depths[r, s] * directions[r] + origins[r]   (formed in registers as lp_render_samples_forward forms it; q = p or, with
 *          contract_coords, the Renderer's contraction of p),  b = grid_idx[r] clamped to the grid-list's batch,
 * the three entry points are the partial derivatives of
 *   T(G, W, F; P) = sum_r sum_s W[r, s] sum over grids g and corners k of  w_k(q_rs) <G_g[row_k(q_rs)], F[r]>
 * with row_k / w_k the corner rows and tri- / bi-linear weights of LpPointGridArgs (align_corners off, zero padding; with
 * mask_out_of_bounds a point outside [-1, 1]^3 -- after the contraction -- contributes nothing at all).  T is the bilinear form B of
 * LpPointGridArgs with U[r, s] = W[r, s] F[r].
 *   lp_ray_grid_splat:        dT/dG: W[r, s] w_k vectors[r, :] is ADDED atomically to row row_k of every grid -- the memory `grid`
 *                             describes is accumulated into and zeroed by the caller.  One wavefront per ray, chunks of 64 samples:
 *                             lane = sample leaves its corner rows and the coefficients W w_k in LDS, then lanes = channels with
 *                             vectors[r] in registers; an atomic instruction covers whole rows of C * 4 bytes.  With row_weight[g] !=
 *                             NULL for EVERY grid, W w_k is also added to row_weight[g][row_k] (zeroed by the caller; the division is
 *                             lp_point_normalize with an LpPointGridArgs of the same grid and row_weight).
 *   lp_ray_grid_gather:       out_features[r, :] = dT/dF = sum_s W[r, s] sum_g sum_k w_k G_g[row_k]  (WRITTEN entirely; one wavefront
 *                             per ray, no atomics, a fixed summation order: bit-reproducible).  With row_weight[g] != NULL a row of grid
 *                             g is divided by max(row_weight[g][row_k], 1e-5) as it is read.  C % 4 == 0: C / 4 lanes per sample, 16
 *                             bytes of a row per lane; else one lane per sample, float by float.  `vectors` is ignored.
 *   lp_ray_grid_grad_samples: grad_weights[r, s] = dT/dW = <vectors[r], sample(G, p_rs)> and grad_depths[r, s] = W[r, s] <dB/dp_rs,
 *                             directions[r]> (dB/dp as lp_point_grad_points forms it, the contraction's Jacobian included; the mask is
 *                             piecewise constant and contributes nothing).  Both WRITTEN entirely, one lane per sample, no atomics;
 *                             either may be NULL (skipped), not both.  row_weight is ignored.
 * row_weight[g] indexes rows as grids[g] does (LpPointGridArgs).  Rows are 64-bit.  1 .. LP_MAX_GRIDS grids, 1 .. LP_MAX_WIDTH
 * channels, any S >= 0 with n_rays * S < 2^31.  No workspace, no allocation, no host synchronisation: graph-capturable.
 * Before anything touches the device: LP_ENULL for NULL args / origins / directions / grid_idx / depths / weights, a grid without data,
 * a NULL vectors (splat, grad_samples), out_features (gather) or both of grad_weights and grad_depths (grad_samples); LP_EINVAL for
 * n_rays < 0, n_samples < 0, a malformed grid-list, channels != grid.channels, row_weight for some grids only (splat), an under-aligned
 * pointer (the message begins with the field); LP_EUNSUPPORTED for channels outside [1, LP_MAX_WIDTH] or n_rays * n_samples >= 2^31.
 * The NULL checks are made whatever n_rays and n_samples are; n_rays * n_samples == 0 then returns LP_OK without a launch (the
 * gather's out_features is the caller's to zero in that case). */
typedef struct LpRayGridArgs {
  LpGridList grid;                 /* read (gather, grad_samples), accumulated into (splat) */
  float* row_weight[LP_MAX_GRIDS]; /* per-grid [rows] fp32 or NULL: read (gather), accumulated into (splat) */
  const float* origins;            /* [n_rays, 3] read */
  const float* directions;         /* [n_rays, 3] read */
  const int32_t* grid_idx;         /* [n_rays] read: batch element of each ray, as LpRays.grid_idx */
  const float* depths;             /* [n_rays, S] read */
  const float* weights;            /* [n_rays, S] read */
  const float* vectors;            /* F [n_rays, C]: the feature to splat / the per-ray vector of grad_samples */
  float* out_features;             /* gather: [n_rays, C] (written) */
  float* grad_weights;             /* grad_samples: [n_rays, S] (written) or NULL */
  float* grad_depths;              /* grad_samples: [n_rays, S] (written) or NULL */
  int64_t n_rays;
  int32_t n_samples;               /* S >= 0 */
  int32_t channels;                /* C of vectors / out_features as the caller laid them out: has to equal grid.channels */
  int32_t mask_out_of_bounds;
  int32_t contract_coords;
} LpRayGridArgs;
int lp_ray_grid_splat(const LpRayGridArgs* args, void* stream);
int lp_ray_grid_gather(const LpRayGridArgs* args, void* stream);
int lp_ray_grid_grad_samples(const LpRayGridArgs* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LIGHTPLANE_HIP_RAY_GRID_H */

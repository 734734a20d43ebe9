/*
 * lightplane_hip_kplanes.h -- space-time plane encoding of 3-D points with a timestamp (the K-Planes / HexPlane field representation;
 * without the time planes, the Hadamard tri-plane), forward and both gradients (lp_kplanes.hip; an extension of lightplane_hip.h,
 * whose Conventions hold here: plain C, fp32, contiguous tensors, 16-byte aligned device pointers, asynchronous calls on `stream`).
 *
 *   out[r, n, s * C + c] = product over the planes j of scale s of:  sum over the 4 vertices k around the point:  w_jk * planes[b, offset[s][j] + row_jk, c]
 *
 * The family is declared here and not in one of the other headers so that their tables stay as they are.  lp_abi_sizeof(50) answers
 * for LpKPlanesArgs; 48, 49 and 51 do not exist.
 */
#ifndef LIGHTPLANE_HIP_KPLANES_H
#define LIGHTPLANE_HIP_KPLANES_H

#include "lightplane_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LP_KPLANES_MAX_SCALES 8
#define LP_KPLANES_MAX_PLANES 6
#define LP_KPLANES_MAX_RESOLUTION 4096

/* The LAYOUT is the caller's (lightplane_amd/kplanes.py: kplanes_layout() computes it); the kernels read it as tables.  There are
 * S = n_scales scales (1 .. 8) of P = n_planes planes each: P = 3, the STATIC variant, planes xy, xz, yz in that order; P = 6, the
 * DYNAMIC variant, followed by xt, yt, zt.  Scale s has n_s = spatial[s] vertices on each of x, y, z and, when dynamic,
 * m_s = temporal[s] vertices on t (both 2 .. 4096).  A plane over the axes (u, v) has n_u * n_v vertices, vertex (i_u, i_v) is row
 * i_u + n_u * i_v, and the plane occupies rows offset[s][j] .. offset[s][j] + n_u * n_v of every batch element; planes do not
 * overlap, follow each other in the order (scale, plane) and end at or below `rows`.  planes is [batch, rows, C] fp32, C = channels
 * in {4, 8, 16, 32, 64}, S * C <= LP_MAX_WIDTH.  Row offsets are 64-bit.
 *
 * Point p = points[r, n] belongs to batch element b = grid_idx[r] clamped to [0, batch).  q = p or, with contract_coords, the
 * Renderer's contraction of p (into [-1, 1]^3).  With mask_out_of_bounds a point whose q lies outside [-1, 1]^3 has all features
 * exactly 0 and exactly zero gradients; time never masks.  Its timestamp is times[r] (time_per_point == 0) or times[r, n]
 * (time_per_point == 1), in [-1, 1].  On an axis of n vertices x = clamp(fma(q, (n - 1) / 2, (n - 1) / 2), 0, n - 1) (one rounding),
 * i = min(floor(x), n - 2), f = x - i -- the same i and f on every plane that holds the axis; the time axis goes through the same map
 * with m_s.  The 4 vertices of plane j are i + {0, 1} on its two axes with the bilinear weights (1 - f | f); v_j is their weighted sum
 * (a C-vector), and the features of the scale are the elementwise product of the P values.  Scales are concatenated scale-major;
 * there is no normalisation.
 *
 *   lp_kplanes_forward:         out_features [n_rays, n_pts, S * C] WRITTEN entirely.  C / 4 lanes per (point, scale), a float4 of
 *                               channels each, the scale the slow workgroup index; the 4 P vertex loads are issued before the first
 *                               use; no LDS, no atomics: bit-reproducible.
 *   lp_kplanes_backward_planes: w_jk * (product of the OTHER planes' values) * grad_features[r, n, s * C + c] is ADDED atomically to
 *                               grad_planes (zeroed by the caller).  One wavefront per 64 consecutive points of a scale: geometry by
 *                               lane = point into LDS, then lanes = channels; each group of C lanes walks its consecutive points and
 *                               keeps, per plane, four vertex sums in registers that it adds (one whole row of C floats per
 *                               instruction) only when the plane's base vertex changes.  The summation order is not fixed.
 *   lp_kplanes_backward_points: grad_points [n_rays, n_pts, 3] WRITTEN entirely: sum over scales and planes of (d v_j / d axis) *
 *                               (product of the other values) * grad_features, times (n_s - 1) / 2, through the contraction's Jacobian
 *                               when asked; 0 on an axis whose x was clamped.  C / 4 lanes per point, no atomics, fixed order:
 *                               bit-reproducible.
 * No derivative divides by a plane value: values may be exactly 0.  Nothing flows to times or grid_idx.  No workspace, no
 * allocation, no host synchronisation: graph-capturable.
 * Before anything touches the device: LP_ENULL for NULL args / points / grid_idx, NULL times with n_planes == 6, a NULL planes
 * (every entry point: the backwards recompute the values), out_features (forward), grad_features (both backwards), grad_planes (backward_planes) or grad_points
 * (backward_points); LP_EINVAL for an under-aligned pointer (the message begins with the field), n_rays < 0, n_pts < 0, batch < 1,
 * n_planes not 3 or 6, times given with n_planes == 3, time_per_point not 0 or 1, n_scales outside [1, 8], a resolution outside
 * [2, 4096] and a layout that breaks a rule above; LP_EUNSUPPORTED for channels outside {4, 8, 16, 32, 64}, S * C > LP_MAX_WIDTH or
 * n_rays * n_pts >= 2^31.  The checks are made whatever n_rays and n_pts are; n_rays * n_pts == 0 then returns LP_OK without a launch. */
typedef struct LpKPlanesArgs {
  const float* planes;                 /* [batch, rows, C] read (forward, both backwards) */
  float* grad_planes;                  /* [batch, rows, C] accumulated into (backward_planes) */
  const float* points;                 /* [n_rays, n_pts, 3] read */
  const float* times;                  /* [n_rays] or [n_rays, n_pts] read (n_planes == 6); NULL (n_planes == 3) */
  const int32_t* grid_idx;             /* [n_rays] read: batch element of each row of points, as LpRays.grid_idx */
  float* out_features;                 /* forward: [n_rays, n_pts, S * C] (written) */
  const float* grad_features;          /* backwards: [n_rays, n_pts, S * C] read */
  float* grad_points;                  /* backward_points: [n_rays, n_pts, 3] (written) */
  int64_t rows;                        /* rows per batch element */
  int64_t n_rays;
  int64_t n_pts;
  int64_t offset[LP_KPLANES_MAX_SCALES][LP_KPLANES_MAX_PLANES]; /* first row of plane j of scale s */
  int32_t spatial[LP_KPLANES_MAX_SCALES];  /* n_s */
  int32_t temporal[LP_KPLANES_MAX_SCALES]; /* m_s (n_planes == 6) */
  int32_t batch;
  int32_t channels;                    /* C */
  int32_t n_scales;                    /* S */
  int32_t n_planes;                    /* P: 3 or 6 */
  int32_t time_per_point;              /* 0: times [n_rays]; 1: times [n_rays, n_pts] */
  int32_t mask_out_of_bounds;
  int32_t contract_coords;
  int32_t reserved;
} LpKPlanesArgs;
int lp_kplanes_forward(const LpKPlanesArgs* args, void* stream);
int lp_kplanes_backward_planes(const LpKPlanesArgs* args, void* stream);
int lp_kplanes_backward_points(const LpKPlanesArgs* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LIGHTPLANE_HIP_KPLANES_H */

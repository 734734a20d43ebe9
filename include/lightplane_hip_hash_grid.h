/*
 * lightplane_hip_hash_grid.h -- multiresolution hash-grid encoding of 3-D points (the Instant-NGP field representation), forward and
 * both gradients (lp_hash_grid.hip; an extension of lightplane_hip.h, whose Conventions hold here: plain C, fp32, contiguous tensors,
 * 16-byte aligned device pointers, asynchronous calls on `stream`).
 *
 *   out[r, n, l * F + c] = sum over the 8 corners k of the cell of level l around q:  w_k * table[b, offset_l + index_l(corner_k), c]
 *
 * The family is declared here and not in one of the other headers so that their tables stay as they are.  lp_abi_sizeof(38) answers
 * for LpHashGridArgs; 36, 37 and 39 do not exist.
 */
#ifndef LIGHTPLANE_HIP_HASH_GRID_H
#define LIGHTPLANE_HIP_HASH_GRID_H

#include "lightplane_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LP_HASH_MAX_LEVELS 32

/* The LAYOUT is the caller's (lightplane_amd/hash_grid.py: hash_grid_layout() computes it in doubles); the kernels read it as tables
 * and compute no growth factor.  Level l has resolution N_l = resolution[l] (1 .. 65536) and a lattice of S_l = N_l + 1 vertices per
 * axis.  hashed[l] == 0: DENSE, entry ix + S_l * (iy + S_l * iz), size[l] = S_l^3 rounded up to a multiple of 8 (S_l^3 <= 2^24).
 * hashed[l] != 0: entry (ix ^ (iy * 2654435761) ^ (iz * 805459861)) & (size[l] - 1) in wrapping uint32 arithmetic, size[l] a power of
 * two in [8, 2^24].  Level l occupies entries offset[l] .. offset[l] + size[l] of every batch element; levels do not overlap, are in
 * increasing order and end at or below `entries`.  table is [batch, entries, F] fp32, F = features_per_level in {1, 2, 4, 8},
 * 1 <= n_levels <= LP_HASH_MAX_LEVELS, n_levels * F <= LP_MAX_WIDTH.  Entry offsets are 64-bit.
 *
 * Point p = points[r, n] belongs to batch element b = grid_idx[r] clamped to [0, batch).  q = p or, with contract_coords, the
 * Renderer's contraction of p (into [-1, 1]^3).  With mask_out_of_bounds a point whose q lies outside [-1, 1]^3 has all features
 * exactly 0 and exactly zero gradients.  Per axis x = clamp(fma(q, N_l / 2, N_l / 2), 0, N_l) (one rounding), i = min(floor(x),
 * N_l - 1), f = x - i; the corners are i + {0, 1} per axis with the trilinear weights (1 - f | f).  Corners that collide in a hashed
 * level simply add.  fp32 coordinates limit a level's interpolation weights to about N_l * 2^-24 cells.
 *
 *   lp_hash_grid_forward:         out_features [n_rays, n_pts, L * F] WRITTEN entirely, channels level-major.  One lane per (point,
 *                                 level), the level the slow workgroup index; the 8 corner loads (4 * F bytes each) are issued before the
 *                                 first use; no LDS, no atomics: bit-reproducible.
 *   lp_hash_grid_backward_table:  w_k * grad_features[r, n, l * F + c] is ADDED atomically to grad_table (zeroed by the caller), same
 *                                 mapping.  Consecutive lanes of a wavefront that share (b, cell) form a run: their products are summed
 *                                 with a segmented wave scan and only the run's first lane issues atomics; a wavefront without a run of
 *                                 two issues them lane by lane.  The summation order of the atomics is not fixed.
 *   lp_hash_grid_backward_points: grad_points [n_rays, n_pts, 3] WRITTEN entirely: sum over levels and corners of (d w_k / d x)
 *                                 <table row, grad_features of the level> N_l / 2, through the contraction's Jacobian when asked; 0 on
 *                                 an axis whose x was clamped.  One lane per point, no atomics: bit-reproducible.
 * Nothing flows to grid_idx.  No workspace, no allocation, no host synchronisation: graph-capturable.
 * Before anything touches the device: LP_ENULL for NULL args / points / grid_idx, a NULL table (forward, backward_points), out_features
 * (forward), grad_features (both backwards), grad_table (backward_table) or grad_points (backward_points); LP_EINVAL for an
 * under-aligned pointer (the message begins with the field), n_rays < 0, n_pts < 0, batch < 1, n_levels outside [1, 32] and a layout
 * that breaks a rule above; LP_EUNSUPPORTED for features_per_level outside {1, 2, 4, 8}, n_levels * F > LP_MAX_WIDTH or
 * n_rays * n_pts >= 2^31.  The checks are made whatever n_rays and n_pts are; n_rays * n_pts == 0 then returns LP_OK without a launch. */
typedef struct LpHashGridArgs {
  const float* table;                  /* [batch, entries, F] read (forward, backward_points) */
  float* grad_table;                   /* [batch, entries, F] accumulated into (backward_table) */
  const float* points;                 /* [n_rays, n_pts, 3] read */
  const int32_t* grid_idx;             /* [n_rays] read: batch element of each row of points, as LpRays.grid_idx */
  float* out_features;                 /* forward: [n_rays, n_pts, L * F] (written) */
  const float* grad_features;          /* backwards: [n_rays, n_pts, L * F] read */
  float* grad_points;                  /* backward_points: [n_rays, n_pts, 3] (written) */
  int64_t entries;                     /* E: entries per batch element */
  int64_t n_rays;
  int64_t n_pts;
  int64_t offset[LP_HASH_MAX_LEVELS];     /* first entry of level l */
  int32_t resolution[LP_HASH_MAX_LEVELS]; /* N_l */
  int32_t size[LP_HASH_MAX_LEVELS];       /* entries of level l */
  int32_t hashed[LP_HASH_MAX_LEVELS];     /* 0 dense, 1 hashed */
  int32_t batch;
  int32_t features_per_level;          /* F */
  int32_t n_levels;                    /* L */
  int32_t mask_out_of_bounds;
  int32_t contract_coords;
  int32_t reserved;
} LpHashGridArgs;
int lp_hash_grid_forward(const LpHashGridArgs* args, void* stream);
int lp_hash_grid_backward_table(const LpHashGridArgs* args, void* stream);
int lp_hash_grid_backward_points(const LpHashGridArgs* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LIGHTPLANE_HIP_HASH_GRID_H */

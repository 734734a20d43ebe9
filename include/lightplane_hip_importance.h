/*
 * lightplane_hip_importance.h -- importance resampling for the march in pieces (lp_importance.hip; an extension of lightplane_hip.h,
 * whose Conventions hold here: plain C, fp32, contiguous tensors, 16-byte aligned device pointers, asynchronous calls on `stream`).
 *
 *   ray_samples -> decoder -> composite (weights) -> importance_samples -> decoder -> composite
 *
 * is the coarse -> fine pass of NeRF: the compositing weights of a coarse march are a histogram over depth, and N new depths are drawn
 * from it by inverting its CDF at stratified targets.  The targets ascend, so the new depths come out sorted and merging them into the
 * coarse ones is a rank computation, not a sort: one wavefront per ray does histogram -> CDF -> inverse -> merge -> deltas -> points
 * with everything in LDS.  fp32, no atomics (bit-reproducible), no workspace, no host synchronisation (graph-capturable), no RNG.
 *
 * The family is declared here and not in lightplane_hip.h or lightplane_hip_samples.h so that the tables of those headers stay as
 * they are.  lp_abi_sizeof(22) answers for LpImportanceArgs; 21 and 23 do not exist.
 *
 * Every buffer below is marked WRITTEN (the kernel writes every element: it may be uninitialised) or read.  Nothing is accumulated
 * into: no buffer has to be zeroed by the caller.
 */
#ifndef LIGHTPLANE_HIP_IMPORTANCE_H
#define LIGHTPLANE_HIP_IMPORTANCE_H

#include "lightplane_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* With S = n_samples coarse depths d_0 <= ... <= d_{S-1} per ray (non-decreasing by contract, not checked), their weights w and
 * N = n_importance, for every ray:
 *   edges    e_0 = d_0,  e_j = (d_{j-1} + d_j) / 2 (0 < j < S),  e_S = d_{S-1}: S bins, bin j the cell around coarse sample j
 *   mass     p_j = max(w_j, 0) + pad (a negative or NaN weight counts as 0),  C_0 = 0,  C_{j+1} = C_j + p_j,  W = C_S
 *   targets  u_k = (k + xi_k) / N,  xi_k = jitter[r, k], or 0.5 with jitter == NULL
 *   bin      j = the last bin with C_j <= u_k W (at most S - 1)
 *   a        = clamp((u_k W - C_j) / (C_{j+1} - C_j), 0, 1), 0 for a zero denominator
 *   t_k      = min(max(e_j + a (e_{j+1} - e_j), e_j), e_{j+1}): non-decreasing in k and inside [d_0, d_{S-1}], in fp32 as well
 * The S' = S + N (include_coarse != 0) or N (include_coarse == 0) result depths are the sorted union of d and t (values copied, never
 * recomputed; of equal values the coarse one comes first), resp. t alone;
 *   delta'_i = depth'_i - depth'_{i-1},  delta'_0 = depth'_1 - depth'_0 (1 when S' = 1),
 *   point'_i = depth'_i * direction + origin  (never contracted: the consumers contract).
 *
 * lp_importance_samples_forward:  out_points / out_depths / out_deltas are WRITTEN entirely (all three are required); origins,
 *                                 directions, depths and weights are required, jitter is optional.  Every input is read once.
 * lp_importance_samples_backward: sample positions are a stop-gradient; the points are differentiable with respect to the ray at
 *                                 fixed depths: grad_origins[r] = sum_i grad_points[r, i], grad_directions[r] = sum_i depth'_i
 *                                 grad_points[r, i], each WRITTEN entirely where non-NULL (NULL = not computed).  directions (only
 *                                 its alignment is looked at: the sums do not depend on it), out_depths (read: the forward's result)
 *                                 and grad_points are required; nothing else is looked at but n_rays, n_samples, n_importance and
 *                                 include_coarse.  One wavefront sums over the samples of one ray: no traffic between rays.
 * Before anything touches the device: LP_ENULL for NULL args or a NULL required pointer; LP_EINVAL for n_rays < 0, n_samples < 2,
 * n_importance < 1, a pad that is not finite or <= 0, or an under-aligned pointer (the message begins with the field);
 * LP_EUNSUPPORTED for n_samples or n_importance above LP_IMPORTANCE_MAX or n_rays * (n_samples + n_importance) >= 2^31.
 * n_rays == 0 returns LP_OK without a launch. */
#define LP_IMPORTANCE_MAX 2048
typedef struct LpImportanceArgs {
  const float* origins;      /* [n_rays, 3] read */
  const float* directions;   /* [n_rays, 3] read */
  const float* depths;       /* [n_rays, S] read: the coarse depths, non-decreasing per ray */
  const float* weights;      /* [n_rays, S] read: anything; negative and NaN entries count as 0 */
  const float* jitter;       /* [n_rays, N] read: in [0, 1); NULL = 0.5 everywhere */
  int64_t n_rays;
  int32_t n_samples;         /* S in [2, LP_IMPORTANCE_MAX] */
  int32_t n_importance;      /* N in [1, LP_IMPORTANCE_MAX] */
  int32_t include_coarse;    /* != 0: S' = S + N, the coarse depths are merged in; 0: S' = N */
  float pad;                 /* > 0, finite: the mass every bin has besides its weight */
  float* out_points;         /* forward: [n_rays, S', 3] WRITTEN entirely */
  float* out_depths;         /* forward: [n_rays, S'] WRITTEN entirely; backward: read */
  float* out_deltas;         /* forward: [n_rays, S'] WRITTEN entirely */
  const float* grad_points;  /* backward: [n_rays, S', 3] read */
  float* grad_origins;       /* backward: [n_rays, 3] WRITTEN entirely, NULL = skip */
  float* grad_directions;    /* backward: [n_rays, 3] WRITTEN entirely, NULL = skip */
} LpImportanceArgs;
int lp_importance_samples_forward(const LpImportanceArgs* args, void* stream);
int lp_importance_samples_backward(const LpImportanceArgs* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LIGHTPLANE_HIP_IMPORTANCE_H */

/*
 * lightplane_hip_losses.h -- per-ray regularisers on the samples of the march in pieces (lp_ray_losses.hip; an extension of
 * lightplane_hip.h, whose Conventions hold here: plain C, fp32, contiguous tensors, 16-byte aligned device pointers, asynchronous
 * calls on `stream`).
 *
 *   ray_samples -> decoder -> composite (weights) -> distortion loss
 *   coarse march (weights) -> importance_samples -> fine march (weights) -> interlevel loss of the coarse weights
 *
 * Both are mip-NeRF 360's regularisers, consumers of the per-sample weights lp_composite_forward hands back.  Each is a scan along
 * the ray: one wavefront per ray, lanes over samples in chunks of 64 with carries between the chunks.  fp32 in and out, no atomics
 * (bit-reproducible), no workspace, no host synchronisation (graph-capturable); the backwards recompute the scans from the inputs.
 *
 * The family is declared here and not in one of the other headers so that their tables stay as they are.  lp_abi_sizeof(24) answers
 * for LpDistortionArgs and lp_abi_sizeof(26) for LpInterlevelArgs; 23, 25 and 27 do not exist.
 *
 * Every buffer below is marked WRITTEN (the kernel writes every element: it may be uninitialised) or read.  Nothing is accumulated
 * into: no buffer has to be zeroed by the caller.
 */
#ifndef LIGHTPLANE_HIP_LOSSES_H
#define LIGHTPLANE_HIP_LOSSES_H

#include "lightplane_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the most samples (and proposal samples) per ray: a ray's working set stays in the 64 KB of LDS a workgroup has without asking */
#define LP_RAY_LOSS_MAX 2048

/* Distortion loss.  With S = n_samples weights w, depths d_0 <= ... <= d_{S-1} (non-decreasing by contract, not checked) and deltas
 * per ray,
 *   L = 2 sum_{i > j} w_i w_j (d_i - d_j) + (1/3) sum_i w_i^2 delta_i
 * which for sorted depths is mip-NeRF 360's sum_ij w_i w_j |d_i - d_j| + (1/3) sum_i w_i^2 delta_i, with a gradient at equal depths.
 * Nothing is clamped: a negative weight is a number.  L does not change when a constant is added to d and is homogeneous of degree 1
 * in (d, delta): the loss on normalised distances is L / (far - near).  Computed in O(S) with
 *   A_i = sum_{j <= i} w_j,  R_i = sum_{j >= i} w_j,  gap_k = d_{k+1} - d_k,
 *   D_i = sum_{k < i} gap_k A_k  (= sum_{j < i} w_j (d_i - d_j)),   E_i = sum_{k >= i} gap_k R_{k+1}  (= sum_{j > i} w_j (d_j - d_i)),
 *   L = 2 sum_i w_i D_i + (1/3) sum_i w_i^2 delta_i
 *   dL/dw_i = 2 (D_i + E_i) + (2/3) w_i delta_i,   dL/dd_i = 2 w_i ((A_i - w_i) - (R_i - w_i)),   dL/ddelta_i = (1/3) w_i^2
 * (for w >= 0 every term of D, E and L is non-negative: nothing cancels).
 *
 * lp_distortion_forward:  loss is WRITTEN entirely (required); weights, depths and deltas are required and read once.
 * lp_distortion_backward: grad_weights / grad_depths / grad_deltas are each WRITTEN entirely where non-NULL (NULL = not computed;
 *                         all three NULL: LP_OK without a launch), as grad_loss[r] times the derivatives above; grad_loss == NULL
 *                         means ones.  weights, depths and deltas are required; loss is not looked at.
 * Before anything touches the device: LP_ENULL for NULL args or a NULL required pointer; LP_EINVAL for n_rays < 0, n_samples < 1 or
 * an under-aligned pointer (the message begins with the field); LP_EUNSUPPORTED for n_samples above LP_RAY_LOSS_MAX or
 * n_rays * n_samples >= 2^31.  n_rays == 0 returns LP_OK without a launch. */
typedef struct LpDistortionArgs {
  const float* weights;    /* [n_rays, S] read */
  const float* depths;     /* [n_rays, S] read: non-decreasing per ray */
  const float* deltas;     /* [n_rays, S] read */
  const float* grad_loss;  /* backward: [n_rays] read; NULL = 1 everywhere */
  float* loss;             /* forward: [n_rays] WRITTEN entirely */
  float* grad_weights;     /* backward: [n_rays, S] WRITTEN entirely, NULL = skip */
  float* grad_depths;      /* backward: [n_rays, S] WRITTEN entirely, NULL = skip */
  float* grad_deltas;      /* backward: [n_rays, S] WRITTEN entirely, NULL = skip */
  int64_t n_rays;
  int32_t n_samples;       /* S in [1, LP_RAY_LOSS_MAX] */
  int32_t reserved;        /* not looked at */
} LpDistortionArgs;
int lp_distortion_forward(const LpDistortionArgs* args, void* stream);
int lp_distortion_backward(const LpDistortionArgs* args, void* stream);

/* Interlevel (proposal) loss, mip-NeRF 360's lossfun_outer.  A target histogram (weights w, depths d: S = n_samples per ray) and a
 * proposal histogram (proposal_weights w^, proposal_depths d^: P = n_proposal per ray), both depth rows non-decreasing (a contract,
 * not checked).  Cell edges as lightplane_hip_importance.h places them, in fp32 so that every comparison below is exact:
 *   e_0 = d_0,  e_j = 0.5f (d_{j-1} + d_j) (0 < j < S),  e_S = d_{S-1};  e^_0 ... e^_P likewise
 *   C^_0 = 0,  C^_{j+1} = C^_j + w^_j
 *   n_k     = #{i in 0..P : e^_i <= e_k}            (k = 0 .. S)
 *   lo_k    = max(0, n_k - 1),  hi_k = min(P, n_{k+1})
 *   bound_k = C^[hi_k] - C^[lo_k]                   (the mass of every proposal bin that touches cell k)
 *   L       = sum_k max(0, w_k - bound_k)^2 / (w_k + eps)
 * w, d and d^ are stop-gradients; with c_k = -2 max(0, w_k - bound_k) / (w_k + eps) and G_n = sum_{k < n} c_k,
 *   dL/dw^_j = G[#{k : lo_k <= j}] - G[#{k : hi_k <= j}]
 * (lo and hi are non-decreasing in k: a contiguous range of cells, two bisections and a difference).  C^ and G are held in fp64.
 *
 * lp_interlevel_forward:  loss is WRITTEN entirely (required); the four inputs are required.
 * lp_interlevel_backward: grad_proposal_weights is WRITTEN entirely (required), as grad_loss[r] times the derivative above;
 *                         grad_loss == NULL means ones.  The four inputs are required; loss is not looked at.
 * Before anything touches the device: LP_ENULL for NULL args or a NULL required pointer; LP_EINVAL for n_rays < 0, n_samples < 2,
 * n_proposal < 2, an eps that is not finite or <= 0, or an under-aligned pointer (the message begins with the field);
 * LP_EUNSUPPORTED for n_samples or n_proposal above LP_RAY_LOSS_MAX or n_rays * max(n_samples, n_proposal) >= 2^31.
 * n_rays == 0 returns LP_OK without a launch. */
typedef struct LpInterlevelArgs {
  const float* weights;           /* [n_rays, S] read */
  const float* depths;            /* [n_rays, S] read: non-decreasing per ray */
  const float* proposal_weights;  /* [n_rays, P] read */
  const float* proposal_depths;   /* [n_rays, P] read: non-decreasing per ray */
  const float* grad_loss;         /* backward: [n_rays] read; NULL = 1 everywhere */
  float* loss;                    /* forward: [n_rays] WRITTEN entirely */
  float* grad_proposal_weights;   /* backward: [n_rays, P] WRITTEN entirely */
  int64_t n_rays;
  int32_t n_samples;              /* S in [2, LP_RAY_LOSS_MAX] */
  int32_t n_proposal;             /* P in [2, LP_RAY_LOSS_MAX] */
  float eps;                      /* > 0, finite */
  int32_t reserved;               /* not looked at */
} LpInterlevelArgs;
int lp_interlevel_forward(const LpInterlevelArgs* args, void* stream);
int lp_interlevel_backward(const LpInterlevelArgs* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LIGHTPLANE_HIP_LOSSES_H */

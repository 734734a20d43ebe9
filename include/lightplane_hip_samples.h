/*
 * lightplane_hip_samples.h -- the ray march as two stand-alone ops (lp_composite.hip; an extension of lightplane_hip.h, whose
 * Conventions hold here: plain C, fp32, contiguous tensors, 16-byte aligned device pointers, asynchronous calls on `stream`).
 *
 *   ray_samples -> (a decoder of the caller's own) -> composite
 *
 * is the Renderer's march with the decoder taken out: lp_ray_samples_* place the samples where the Renderer's kernels place theirs
 * (the same device functions compute them), lp_composite_* integrate opacities and features along each ray as the Renderer does.
 * Every kernel is fp32, uses no atomics (bit-reproducible), no workspace and no host synchronisation (graph-capturable).
 *
 * The family is declared here and not in lightplane_hip.h so that the tables of that header (its prototypes, lp_build_info(),
 * LP_VERSION) stay as they are.  lp_abi_sizeof(18) answers for LpRaySamplesArgs and lp_abi_sizeof(20) for LpCompositeArgs; 19 and 21
 * do not exist.
 *
 * Every buffer below is marked WRITTEN (the kernel writes every element: it may be uninitialised) or read.  Nothing is accumulated
 * into: no buffer has to be zeroed by the caller.
 */
#ifndef LIGHTPLANE_HIP_SAMPLES_H
#define LIGHTPLANE_HIP_SAMPLES_H

#include "lightplane_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Sample placement.  With S = march.num_samples, S_inf = march.num_samples_inf, S_tot = S + S_inf and, for ray r,
 *   depth[r, i] = near + linspace(0, 1, S)[i] (far - near)                       i <  S   (the two-sided linspace of the Renderer)
 *               = far * (float)(1 / ((disparity_at_inf - 1) (k + 1) / S_inf + 1))  i = S + k (double arithmetic, one cast)
 *   delta[r, 0] = (far - near) / (S - 1), or 1 when S = 1;   delta[r, i] = depth[r, i] - depth[r, i - 1]
 *   point[r, i] = depth[r, i] * direction[r] + origin[r]                          (never contracted: the consumers contract)
 * march.mask_out_of_bounds and march.contract_coords are not looked at.
 *
 * lp_ray_samples_forward:  points / depths / deltas are WRITTEN entirely (all three are required).
 * lp_ray_samples_backward: the vector-Jacobian product of the above.  grad_points / grad_depths / grad_deltas are the upstream
 *                          gradients (read; NULL = zeros); grad_origins / grad_directions / grad_near / grad_far are WRITTEN
 *                          entirely where non-NULL (NULL = not computed).  One wavefront sums over the samples of one ray: no
 *                          traffic between rays.  points / depths / deltas are not looked at.
 * rays.origins / directions / near_t / far_t are required (with n_rays > 0); rays.grid_idx and rays.encoding are not read and may
 * be NULL.  Before anything touches the device: LP_ENULL for NULL args or a NULL required pointer; LP_EINVAL for n_rays < 0,
 * num_samples < 1, num_samples_inf < 0 or an under-aligned pointer (the message begins with the field); LP_EUNSUPPORTED for
 * n_rays * S_tot >= 2^31.  n_rays == 0 returns LP_OK without a launch. */
typedef struct LpRaySamplesArgs {
  LpRays rays;                  /* read: origins, directions, near_t, far_t */
  LpMarch march;                /* num_samples, num_samples_inf, disparity_at_inf */
  float* points;                /* forward: [n_rays, S_tot, 3] WRITTEN entirely */
  float* depths;                /* forward: [n_rays, S_tot]    WRITTEN entirely */
  float* deltas;                /* forward: [n_rays, S_tot]    WRITTEN entirely */
  const float* grad_points;     /* backward: [n_rays, S_tot, 3] read, NULL = zeros */
  const float* grad_depths;     /* backward: [n_rays, S_tot]    read, NULL = zeros */
  const float* grad_deltas;     /* backward: [n_rays, S_tot]    read, NULL = zeros */
  float* grad_origins;          /* backward: [n_rays, 3] WRITTEN entirely, NULL = skip */
  float* grad_directions;       /* backward: [n_rays, 3] WRITTEN entirely, NULL = skip */
  float* grad_near;             /* backward: [n_rays]    WRITTEN entirely, NULL = skip */
  float* grad_far;              /* backward: [n_rays]    WRITTEN entirely, NULL = skip */
} LpRaySamplesArgs;
int lp_ray_samples_forward(const LpRaySamplesArgs* args, void* stream);
int lp_ray_samples_backward(const LpRaySamplesArgs* args, void* stream);

/* Emission-absorption compositing of S = n_samples samples per ray, C = channels feature channels.  With od_s = opacity_s delta_s
 * (opacity: a density, >= 0 by contract, not clamped), N_s = sum_{j < s} od_j, T_s = exp(-N_s), w_s = T_s - T_{s+1}, computed as
 * T_s (-expm1(-od_s)):
 *   ray_length[r] = sum_s w_s depth_s,   neg_log_t[r] = N_S,   feature[r, :] = sum_s w_s features[r, s, :],   weights[r, s] = w_s
 * -- the Renderer's three outputs in the Renderer's order.  One wavefront per ray; prefix sums are wave scans with a carry between
 * chunks of 64 samples; the ray's S * C features are streamed contiguously, 16 bytes per lane where C % 4 == 0.
 *
 * lp_composite_forward:  ray_length / neg_log_t are WRITTEN entirely (required), feature is WRITTEN entirely (required when
 *                        channels > 0), weights is WRITTEN entirely where non-NULL.  Every input is read once.
 * lp_composite_backward: recomputes the scan from the inputs (nothing of the forward is kept).  grad_ray_length / grad_neg_log_t /
 *                        grad_feature / grad_weights are the upstream gradients (read; NULL = zeros); with
 *                        v_s = grad_ray_length depth_s + <grad_feature, features_s> + grad_weights_s and
 *                        d_j = T_{j+1} v_j - sum_{s > j} w_s v_s + grad_neg_log_t:
 *                          grad_opacity_j = d_j delta_j,   grad_deltas_j = d_j opacity_j,   grad_depths_s = grad_ray_length w_s,
 *                          grad_features[s, c] = w_s grad_feature[c]
 *                        each WRITTEN entirely where non-NULL (NULL = not computed).  opacity and deltas are read twice (a ray
 *                        of more than 32 768 samples is done in blocks of that many from the far end, and they are read once
 *                        more per block), everything else once; `features` is read only when grad_feature is given and
 *                        grad_opacity or grad_deltas is asked for.
 *                        The forward's outputs are not looked at.
 * opacity / depths / deltas are required, and features when channels > 0 (with n_rays > 0).  T_s underflowing to 0 and rows of zero
 * opacity give finite results and gradients.  Before anything touches the device: LP_ENULL for NULL args or a NULL required pointer;
 * LP_EINVAL for n_rays < 0, n_samples < 1 or an under-aligned pointer (the message begins with the field); LP_EUNSUPPORTED for channels
 * outside [0, LP_MAX_WIDTH] or n_rays * n_samples >= 2^31.  n_rays == 0 returns LP_OK without a launch. */
typedef struct LpCompositeArgs {
  const float* opacity;          /* [n_rays, S]    read */
  const float* features;         /* [n_rays, S, C] read; NULL with channels == 0 */
  const float* depths;           /* [n_rays, S]    read */
  const float* deltas;           /* [n_rays, S]    read */
  int64_t n_rays;
  int32_t n_samples;             /* S >= 1 */
  int32_t channels;              /* C in [0, LP_MAX_WIDTH], any value */
  float* ray_length;             /* forward: [n_rays]    WRITTEN entirely */
  float* neg_log_t;              /* forward: [n_rays]    WRITTEN entirely */
  float* feature;                /* forward: [n_rays, C] WRITTEN entirely (channels > 0) */
  float* weights;                /* forward: [n_rays, S] WRITTEN entirely, NULL = skip */
  const float* grad_ray_length;  /* backward: [n_rays]    read, NULL = zeros */
  const float* grad_neg_log_t;   /* backward: [n_rays]    read, NULL = zeros */
  const float* grad_feature;     /* backward: [n_rays, C] read, NULL = zeros */
  const float* grad_weights;     /* backward: [n_rays, S] read, NULL = zeros */
  float* grad_opacity;           /* backward: [n_rays, S]    WRITTEN entirely, NULL = skip */
  float* grad_features;          /* backward: [n_rays, S, C] WRITTEN entirely, NULL = skip */
  float* grad_depths;            /* backward: [n_rays, S]    WRITTEN entirely, NULL = skip */
  float* grad_deltas;            /* backward: [n_rays, S]    WRITTEN entirely, NULL = skip */
} LpCompositeArgs;
int lp_composite_forward(const LpCompositeArgs* args, void* stream);
int lp_composite_backward(const LpCompositeArgs* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LIGHTPLANE_HIP_SAMPLES_H */

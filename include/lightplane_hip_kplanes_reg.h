/*
 * lightplane_hip_kplanes_reg.h -- the three regularisers of a K-Planes field on the plane layout of lightplane_hip_kplanes.h, value
 * and gradient in one sweep (lp_kplanes_reg.hip; an extension of lightplane_hip.h, whose Conventions hold here: plain C, fp32,
 * contiguous tensors, 16-byte aligned device pointers, asynchronous calls on `stream`).
 *
 * With X_{s,j}[b, i_v, i_u, c] = planes[b, offset[s][j] + i_u + n_u * i_v, c] (planes 0-2: xy, xz, yz with n_u = n_v = spatial[s];
 * planes 3-5: xt, yt, zt with n_u = spatial[s] on the spatial axis and n_v = temporal[s] on the time axis), phi_1(d) = |d| and
 * phi_2(d) = d^2:
 *
 *   terms[0] space_tv        = sum over the planes and their SPATIAL axes a of  mean over the adjacent pairs along a of
 *                              phi_p(X[.. i + 1 ..] - X[.. i ..])                     (both axes of xy / xz / yz, the u axis of xt / yt / zt)
 *   terms[1] time_smoothness = sum over xt / yt / zt of  mean over 1 <= i_v <= n_v - 2 of (X[i_v + 1] - 2 X[i_v] + X[i_v - 1])^2
 *                              (a plane with n_v == 2 has no such triple and contributes exactly 0)
 *   terms[2] time_l1         = sum over xt / yt / zt of  mean of |1 - X|
 *
 * Every mean runs over all batch elements and channels of its (plane, axis).  Pairs never cross a plane, a batch element or the end of
 * an i_v row.  The derivative of |d| at 0 is 0.  A static layout (n_planes == 3) has terms[1] == terms[2] == 0.
 *
 * The family is declared here and not in one of the other headers so that their tables stay as they are.  lp_abi_sizeof(62) answers
 * for LpKPlanesRegArgs; 60, 61 and 63 do not exist.
 */
#ifndef LIGHTPLANE_HIP_KPLANES_REG_H
#define LIGHTPLANE_HIP_KPLANES_REG_H

#include "lightplane_hip_kplanes.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The layout fields are those of LpKPlanesArgs and are held to the same rules.
 *
 *   lp_kplanes_reg_workspace_bytes: bytes of device workspace a call that computes `terms` takes for this layout and batch: three
 *                                   doubles per workgroup of the sweep.  Shapes only: no pointer is looked at, no device is touched.
 *                                   0 with lp_last_error() set where the layout is refused.
 *   lp_kplanes_reg_forward:         terms [3] WRITTEN.
 *   lp_kplanes_reg_backward:        grad_planes [batch, rows, C]: every row of a plane is WRITTEN (accumulate == 0) or ADDED TO
 *                                   (accumulate != 0) with  sum_k weights[k] * grad_terms[k] * d terms[k] / d planes;  rows of no
 *                                   plane (gaps of the layout) are not touched.  grad_terms: [3] in DEVICE memory, NULL = (1, 1, 1).
 *   lp_kplanes_reg_fused:           both in the same sweep.
 *
 * One launch of the sweep for all batch elements, scales and planes, then (where terms are asked for) one small launch that sums
 * the workgroups' partials in fp64 in a fixed order.  No atomics: every gradient element is computed from its stencil and stored
 * once; two calls give the same bits.  No allocation, no host synchronisation: graph-capturable.
 * Before anything touches the device: LP_ENULL for NULL args, planes, terms (forward, fused), grad_planes (backward, fused) or a
 * workspace that is NULL where bytes are needed; LP_EINVAL for an under-aligned pointer (the message begins with the field), p not 1
 * or 2, grad_planes == planes, a workspace smaller than lp_kplanes_reg_workspace_bytes(), batch < 1, n_planes not 3 or 6, n_scales
 * outside [1, 8], a resolution outside [2, 4096] and a layout that breaks a rule of lightplane_hip_kplanes.h; LP_EUNSUPPORTED for
 * channels outside {4, 8, 16, 32, 64}, S * C > LP_MAX_WIDTH or more than 2^31 - 1 workgroups. */
typedef struct LpKPlanesRegArgs {
  const float* planes;                 /* [batch, rows, C] read */
  float* grad_planes;                  /* [batch, rows, C] written or added to (backward, fused) */
  float* terms;                        /* [3] written (forward, fused): space_tv, time_smoothness, time_l1 */
  const float* grad_terms;             /* [3] DEVICE memory, read (backward, fused); NULL = (1, 1, 1) */
  int64_t rows;                        /* rows per batch element */
  int64_t offset[LP_KPLANES_MAX_SCALES][LP_KPLANES_MAX_PLANES]; /* first row of plane j of scale s */
  int32_t spatial[LP_KPLANES_MAX_SCALES];  /* n_s */
  int32_t temporal[LP_KPLANES_MAX_SCALES]; /* m_s (n_planes == 6) */
  float weights[3];                    /* HOST factors of the three terms' gradients (backward, fused) */
  int32_t batch;
  int32_t channels;                    /* C */
  int32_t n_scales;                    /* S */
  int32_t n_planes;                    /* P: 3 or 6 */
  int32_t p;                           /* 1: |d|, 2: d^2 (space_tv) */
  int32_t accumulate;                  /* backward, fused: 0 writes grad_planes, otherwise adds to it */
  int32_t reserved;
} LpKPlanesRegArgs;
int64_t lp_kplanes_reg_workspace_bytes(const LpKPlanesRegArgs* args);
int lp_kplanes_reg_forward(const LpKPlanesRegArgs* args, void* workspace, int64_t workspace_bytes, void* stream);
int lp_kplanes_reg_backward(const LpKPlanesRegArgs* args, void* stream);
int lp_kplanes_reg_fused(const LpKPlanesRegArgs* args, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LIGHTPLANE_HIP_KPLANES_REG_H */

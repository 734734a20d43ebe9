/*
 * lightplane_hip_kplanes_scaffold.h -- the occupancy scaffold of a space-time plane field (K-Planes / HexPlane; without time planes
 * the Hadamard tri-plane) over a set of timestamps: the decoder's opacity on a regular lattice, its maximum over the timestamps,
 * thresholded and dilated, in one lattice launch (lp_kplanes_scaffold.hip; an extension of lightplane_hip_kplanes.h, whose layout
 * rules and encoding hold here, and of lp_scaffold_* of lightplane_hip.h, whose lattice, decoder rule and dilation hold here: plain
 * C, fp32, contiguous tensors, 16-byte aligned device pointers, asynchronous calls on `stream`).
 *
 *   p[z, y, x]          = (lin(W)[x], lin(H)[y], lin(D)[z]),  lin(n) = linspace(0, 1, n) * 2 - 1 (the lattice of lp_scaffold_*)
 *   feat(p, t)[0 .. S C) = the plane encoding of p at the timestamp t (lp_kplanes_forward: batch element b, no contraction, no mask)
 *   opacity[b, z, y, x] = max over t in times of  gain * softplus(opacity MLP(ReLU(trunk MLP(feat(p, t)))))
 *                         (ReLU(feat) without trunk layers; a static layout, n_planes == 3, has no times: one evaluation)
 *   scaffold            = max_pool3d(opacity, 2 r + 1, stride 1, padding r) > threshold  as 0 / 1 floats, r = dilate
 *
 * Every lattice point lies inside [-1, 1]^3, and a scaffold is looked up at the already contracted coordinate: there is neither a
 * mask nor a contraction.  A timestamp outside [-1, 1] clamps as in the encoding.  The colour MLP is never read.
 * The family is declared here and not in one of the other headers so that their tables stay as they are.  lp_abi_sizeof(66) answers
 * for LpKPlanesScaffoldArgs; 64, 65 and 67 do not exist.
 */
#ifndef LIGHTPLANE_HIP_KPLANES_SCAFFOLD_H
#define LIGHTPLANE_HIP_KPLANES_SCAFFOLD_H

#include "lightplane_hip_kplanes.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One wavefront = one workgroup = up to 64 consecutive x of ONE lattice row (b, z, y).  The yz value (once per workgroup) and the
 *   yt and zt values (once per timestamp) are the same for the whole row: lanes = channels form them into LDS vectors [S C].  The xy,
 *   xz and xt values are gathered with lanes = channels (whole plane rows per access), multiplied in the encoding's order
 *   ((((xy xz) yz) xt) yt) zt and written to the decoder's LDS column tile; lane = point runs trunk and opacity head and keeps the
 *   running maximum in a register.  The loop over the timestamps is inside the kernel; (xy xz) yz is formed again per timestamp
 *   (a tile that kept it would cost LDS occupancy: DESIGN.md 4.29).
 * lp_kplanes_scaffold_opacity: opacity [B, D, H, W] WRITTEN entirely (threshold and dilate ignored).
 * lp_kplanes_scaffold_build:   scaffold [B, D, H, W] WRITTEN entirely, through `workspace` (lp_kplanes_scaffold_workspace_bytes:
 *   one byte per lattice point when dilate > 0, else 0 and the workspace may be NULL) and the separable byte dilation of
 *   lp_scaffold_build.  The loop over the timestamps of a wavefront ends once all of its points are above the threshold: the
 *   result is the same bits.
 * No atomics: bit-reproducible.  No allocation, no host synchronisation: graph-capturable.  Row offsets are 64-bit.
 * Before anything touches the device: LP_ENULL for NULL args / planes / mlp_params / the result, or NULL times with n_planes == 6;
 * LP_EINVAL for an under-aligned pointer (the message begins with the field), a layout that breaks a rule of
 * lightplane_hip_kplanes.h (times given with n_planes == 3 is one), MLPs that do not chain from S * C inputs or do not fit
 * n_mlp_params, shape.B != batch, an extent < 1, n_times < 1 with n_planes == 6, dilate < 0, a NaN threshold, or (build) a workspace
 * that is missing, too small, under-aligned or overlaps the result; LP_EUNSUPPORTED for channels outside {4, 8, 16, 32, 64},
 * S * C > LP_MAX_WIDTH, widths outside [1, LP_MAX_WIDTH] or B * D * H * W >= 2^31. */
typedef struct LpKPlanesScaffoldArgs {
  const float* planes;                 /* [batch, rows, C] read */
  const float* times;                  /* [n_times] read on the device (n_planes == 6); NULL (n_planes == 3) */
  int64_t rows;                        /* rows per batch element */
  int64_t offset[LP_KPLANES_MAX_SCALES][LP_KPLANES_MAX_PLANES]; /* the layout: as in LpKPlanesArgs */
  int32_t spatial[LP_KPLANES_MAX_SCALES];
  int32_t temporal[LP_KPLANES_MAX_SCALES];
  int32_t batch;
  int32_t channels;                    /* C */
  int32_t n_scales;                    /* S */
  int32_t n_planes;                    /* P: 3 or 6 */
  int32_t n_times;                     /* T >= 1 (n_planes == 6); ignored otherwise */
  int32_t dilate;                      /* radius r of the dilation window 2 r + 1; 0 = none */
  const float* mlp_params;             /* the decoder's flat parameter vector: trunk | opacity (| colour, never read) */
  int64_t n_mlp_params;
  LpMlp trunk, opacity;                /* as in LpScaffoldArgs; the trunk (without one: the opacity head) reads S * C inputs */
  float gain;
  float threshold;                     /* occupied: opacity > threshold */
  LpGrid shape;                        /* B, D, H, W of the scaffold (row_offset and data ignored) */
} LpKPlanesScaffoldArgs;
int64_t lp_kplanes_scaffold_workspace_bytes(const LpKPlanesScaffoldArgs* args);
int lp_kplanes_scaffold_opacity(const LpKPlanesScaffoldArgs* args, float* opacity, void* stream);
int lp_kplanes_scaffold_build(const LpKPlanesScaffoldArgs* args, float* scaffold, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LIGHTPLANE_HIP_KPLANES_SCAFFOLD_H */

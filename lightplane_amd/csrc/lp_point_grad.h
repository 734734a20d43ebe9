// lp_point_grad.h -- a point of a [n_rays, n_pts, 3] array as the Renderer sees a sample, and the derivative of the grid-list gather with
// respect to it: shared by the decoder at points (lp_points.hip) and the plain gather / splat at points (lp_point_grid.hip).
#pragma once
#include "lp_device.h"

namespace lp {

// The point as the Renderer sees a sample: a ray that starts there, marched to depth 0 (sample_point contracts it when asked).
LP_DEV Ray point_ray(const float* __restrict__ points, int64_t q, int b) {
  Ray r;
  r.ox = points[3 * q + 0];
  r.oy = points[3 * q + 1];
  r.oz = points[3 * q + 2];
  r.dx = r.dy = r.dz = 0.0f;
  r.near_t = r.far_t = 0.0f;
  r.b = b;
  return r;
}

// (a batch index outside the grid-list would address another tensor: clamped, like every other index the kernels form)
LP_DEV int clamp_batch(int b, int B) { return b < 0 ? 0 : (b >= B ? B - 1 : b); }

// d L / d (x, y, z) of the gather of one grid-list: sum over grids and corners of (d w_k / d coordinate) <row_k, d>, d = the gradient
// with respect to the summed features.  w_k is the product of the per-axis weights (1 - f | f), f = t - floor(t), t = ((c + 1) size -
// 1) / 2: d f / d c = size / 2.  A corner outside its grid holds the padding value 0 and contributes nothing.
LP_DEV void point_grad_list(const LpGridList& gl, int b, float x, float y, float z, bool mask_oob, const float* d, float& gx, float& gy,
                            float& gz) {
  if (mask_oob && !point_in_bounds(x, y, z)) return;
  const int C = gl.channels;
  for (int g = 0; g < gl.n_grids; ++g) {
    const LpGrid& gd = gl.grids[g];
    const bool sx = gd.W > 1, sy = gd.H > 1, sz = gd.D > 1;
    const bool voxel = sx && sy && sz;
    const Corners cs = grid_corners<false>(gd, b, x, y, z);
    Axis ax{0, 1.0f, 0.0f}, ay{0, 1.0f, 0.0f}, az{0, 1.0f, 0.0f};
    if (sx) ax = axis_setup<false>(x, gd.W);
    if (sy) ay = axis_setup<false>(y, gd.H);
    if (sz) az = axis_setup<false>(z, gd.D);
    const float hx = sx ? 0.5f * (float)gd.W : 0.0f, hy = sy ? 0.5f * (float)gd.H : 0.0f, hz = sz ? 0.5f * (float)gd.D : 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (k < cs.n && cs.row[k] >= 0) {
        int ux, uy, uz;  // (grid_corners' map of the corner bits onto the sampled axes)
        if (voxel) {
          ux = k & 1; uy = (k >> 1) & 1; uz = (k >> 2) & 1;
        } else if (!sz) {
          ux = k & 1; uy = (k >> 1) & 1; uz = 0;
        } else if (!sy) {
          ux = k & 1; uy = 0; uz = (k >> 1) & 1;
        } else {
          ux = 0; uy = k & 1; uz = (k >> 1) & 1;
        }
        const float* src = gd.data + cs.row[k] * C;
        float dot = 0.0f;
        for (int c = 0; c < C; ++c) dot = fmaf(src[c], d[c], dot);
        const float wx = sx ? (ux ? ax.w_hi : ax.w_lo) : 1.0f;
        const float wy = sy ? (uy ? ay.w_hi : ay.w_lo) : 1.0f;
        const float wz = sz ? (uz ? az.w_hi : az.w_lo) : 1.0f;
        gx = fmaf(dot, (ux ? hx : -hx) * wy * wz, gx);
        gy = fmaf(dot, wx * (uy ? hy : -hy) * wz, gy);
        gz = fmaf(dot, wx * wy * (uz ? hz : -hz), gz);
      }
    }
  }
}

// (gx, gy, gz): gradient with respect to the contracted point q = contract(p) / 2 -> with respect to p (sample_point's contraction:
// n = max |p_j|; n <= 1: q = p / 2; else the coordinates within 1e-7 of n become (2 - 1 / |p_j|) sign(p_j), the others p_j / n).
LP_DEV void contract_backward(float px, float py, float pz, float& gx, float& gy, float& gz) {
  const float ax = fabsf(px), ay = fabsf(py), az = fabsf(pz);
  const float n = fmaxf(fmaxf(ax, ay), az);
  if (!(n <= 1.0f)) {
    const bool mx = fabsf(ax - n) <= 1e-7f, my = fabsf(ay - n) <= 1e-7f, mz = fabsf(az - n) <= 1e-7f;
    const float rn = 1.0f / n;
    // through n = |p_i|, i the first coordinate that attains the maximum: d (p_j / n) / d p_i = -p_j / n^2 * sign(p_i)
    const float dn = -((mx ? 0.0f : gx * px) + (my ? 0.0f : gy * py) + (mz ? 0.0f : gz * pz)) * rn * rn;
    gx = gx * (mx ? 1.0f / (ax * ax) : rn);
    gy = gy * (my ? 1.0f / (ay * ay) : rn);
    gz = gz * (mz ? 1.0f / (az * az) : rn);
    if (ax == n) gx += px < 0.0f ? -dn : dn;
    else if (ay == n) gy += py < 0.0f ? -dn : dn;
    else gz += pz < 0.0f ? -dn : dn;
  }
  gx *= 0.5f;
  gy *= 0.5f;
  gz *= 0.5f;
}

}  // namespace lp

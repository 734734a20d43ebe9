// lp_ray_clip.hip -- clip rays to the occupied span of a scaffold: per ray the sub-interval [near', far'] of [near, far] outside which
// the Renderer's scaffold lookup (scaffold_lookup, lp_device.h) returns 0 for every sample.
//
// One lane = one ray, one wave = one workgroup.  The scaffold is read the way the Renderer reads it -- nearest neighbour,
// align_corners = False --, so scene b is tiled by W x H x D axis-aligned boxes, cell i along x covering [-1 + 2 i / W, -1 + 2 (i + 1) / W],
// and the ray crosses them in a 3-D DDA (Amanatides-Woo):
//   1. slab test against [-1, 1]^3 and [near, far]: the overlap [t0, t1], or a miss.  An axis with d_a == 0 takes no part: the ray
//      stays in the slab the Renderer's own index formula puts o_a in.
//   2. without a scaffold the overlap is the answer.
//   3. forward walk from t0 to the first occupied cell: near*.  None: a miss.
//   4. backward walk from t1 -- the same routine on the reversed ray (o, -d) over [-t1, -t0] -- to the first occupied cell: far*.
//   5. every crossing parameter comes from its plane index, (plane - o_a) / d_a with plane = (2 p - W) / W: nothing is accumulated, so
//      the error does not grow with the number of steps.
//   6. near' = max(near, near* - pad_t - e), far' = min(far, far* + pad_t + e), pad_t = pad * h / |d|, h = 2 / max(D, H, W) (2 without a
//      scaffold).
// e_a = 14 * 2^-24 * (1 + |o_a|) / |d_a| bounds, in ray parameter, how far the Renderer's fp32 sample point (depth * d + o, then the
// un-normalisation) and this kernel's fp32 crossing can disagree about the side of a plane of axis a a sample is on (DESIGN.md 4.13
// has the sum).  A walk stops with the e of the axis it crossed last.  In every cell the walk asks which planes a sample of that stay
// may lie beyond: ahead, a crossing that falls into the stay when taken e_a early; behind, the last crossing of an axis when taken
// e_a late.  More than the next plane alone is rare (an edge, a corner, an axis the ray runs along within rounding): the sample points
// may then be in any of the cells those planes lead to, and the walk looks at all of them (at most 26) before it steps or ends.
// The walks' loops run on an integer counter of at most W + H + D + 2 trips; every scaffold index is range-checked before the read.
// No atomics, no workspace, no LDS; a lane reads its near / far before it writes them, so the results may alias the inputs.
#include "lp_device.h"
#include "lp_host.h"

namespace lp {

constexpr int RC_THREADS = 64;
constexpr float RC_EPS = 14.0f * 5.9604644775390625e-8f;  // 14 * 2^-24

struct RcArgs {
  LpRays rays;
  const float* scaffold;  // NULL: the box only
  int32_t B, D, H, W;
  float pad;
  float* near_out;
  float* far_out;
  uint8_t* hit_out;
};

struct RcWalk {
  const float* scaffold;  // already offset to scene b
  int n[3];               // W, H, D
  float o[3], d[3], e[3];
  bool moving[3];
};

LP_DEV bool rc_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }  // false for NaN and +-Inf

// parameter at which the ray crosses plane p (0 .. n) of axis a
LP_DEV float rc_cross(const RcWalk& w, int a, int p) {
  const float plane = (float)(2 * p - w.n[a]) / (float)w.n[a];
  return (plane - w.o[a]) / w.d[a];
}
// ... at which it leaves / enters cell i of axis a
LP_DEV float rc_exit(const RcWalk& w, int a, int i) { return rc_cross(w, a, w.d[a] > 0.0f ? i + 1 : i); }
LP_DEV float rc_enter(const RcWalk& w, int a, int i) { return rc_cross(w, a, w.d[a] > 0.0f ? i : i + 1); }

LP_DEV bool rc_occupied(const RcWalk& w, int ix, int iy, int iz) {
  if (ix < 0 || ix >= w.n[0] || iy < 0 || iy >= w.n[1] || iz < 0 || iz >= w.n[2]) return false;
  return w.scaffold[((int64_t)iz * w.n[1] + iy) * w.n[0] + ix] != 0.0f;
}

// First occupied cell along the ray within [t0, t1]: true, with the parameter the ray enters it at (t_star, >= t0) and the e of that
// crossing (e_star).  `c`: the cell of every axis that does not move (the others are found here).
LP_DEV bool rc_walk(const RcWalk& w, float t0, float t1, const int* c, float& t_star, float& e_star) {
  int cell[3], step[3];
  float t_prev[3];  // where the ray entered its present cell of each axis
  bool live[3];     // the axis still has a plane of the box ahead
  for (int a = 0; a < 3; ++a) {
    cell[a] = c[a];
    step[a] = 0;
    t_prev[a] = 0.0f;
    live[a] = w.moving[a];
    if (!w.moving[a]) continue;
    step[a] = w.d[a] > 0.0f ? 1 : -1;
    const float p = fmaf(t0, w.d[a], w.o[a]);
    const float f = floorf((p + 1.0f) * 0.5f * (float)w.n[a]);
    int i = f >= (float)(w.n[a] - 1) ? w.n[a] - 1 : (f >= 0.0f ? (int)f : 0);  // (NaN -> 0)
    for (int k = 0; k < 3; ++k) {  // the floor is off by at most one cell: settle it with the crossings the walk itself uses
      const int fwd = i + step[a], bwd = i - step[a];
      if (fwd >= 0 && fwd < w.n[a] && rc_exit(w, a, i) <= t0) i = fwd;
      else if (bwd >= 0 && bwd < w.n[a] && rc_enter(w, a, i) > t0) i = bwd;
    }
    cell[a] = i;
    t_prev[a] = rc_enter(w, a, i);
  }
  // (every array index below is a compile-time constant once the loops over the axes are unrolled: a per-lane array indexed with a
  // run-time value would live in scratch memory)
  float t_cur = t0, e_cur = 0.0f;  // (t0 is near itself or a face of the box with its e already taken off)
  int last = 0;                    // the axis crossed last, as a bit (none yet)
  const int trips = w.n[0] + w.n[1] + w.n[2] + 2;
  for (int trip = 0; trip < trips; ++trip) {
    if (rc_occupied(w, cell[0], cell[1], cell[2])) {
      t_star = t_cur;
      e_star = e_cur;
      return true;
    }
    float tx[3];
    int m = -1;
    float tm = 0.0f, em = 0.0f;
    for (int a = 0; a < 3; ++a) {
      tx[a] = live[a] ? rc_exit(w, a, cell[a]) : 0.0f;
      if (live[a] && (m < 0 || tx[a] < tm)) m = a, tm = tx[a], em = w.e[a];
    }
    if (m < 0) return false;  // no axis has a plane ahead: the ray never leaves this cell
    // The ray stays in this cell over [t_cur, min(t1, tm)]; the Renderer's rounded sample points of that stay may sit
    //   AHEAD of the plane of axis a the ray crosses next, when that crossing taken e_a early falls into the stay (widened by em) --
    //          the next crossing itself and every crossing tied with it (an edge, a corner), also a crossing that lies beyond t1 by
    //          less than its e;
    //   BEHIND the plane of axis a the ray crossed last, when that crossing taken e_a late falls into the stay -- an axis the ray runs
    //          along within rounding keeps its old side possible for many cells of the other axes.
    // The cell the ray came from (behind the axis crossed last, alone) has been looked at, and the next cell alone is the next trip's.
    // Anything more is rare: then every cell the planes in question lead to (at most 26) is looked at before the walk steps or ends.
    const float t_end = fminf(t1, tm + em);
    int ahead = 0, behind = 0;
    float e_tie = 0.0f;
    for (int a = 0; a < 3; ++a) {
      if (live[a] && tx[a] - w.e[a] <= t_end) {
        ahead |= 1 << a;
        e_tie = fmaxf(e_tie, w.e[a]);
      }
      if (w.moving[a] && t_prev[a] + w.e[a] >= t_cur) behind |= 1 << a;
    }
    if ((behind & ~last) != 0 || (ahead & ~(1 << m)) != 0) {
      bool any_behind = false, any_ahead = false;
      for (int s = 0; s < 27; ++s) {
        const int k[3] = {s % 3 - 1, (s / 3) % 3 - 1, s / 9 - 1};  // offsets in steps: -1 behind, +1 ahead
        bool allowed = s != 13, uses_behind = false;
        for (int a = 0; a < 3; ++a) {
          allowed = allowed && (k[a] == 0 || (k[a] > 0 ? (ahead >> a) & 1 : (behind >> a) & 1));
          uses_behind = uses_behind || k[a] < 0;
        }
        if (!allowed) continue;
        const bool occ = rc_occupied(w, cell[0] + k[0] * step[0], cell[1] + k[1] * step[1], cell[2] + k[2] * step[2]);
        any_behind = any_behind || (occ && uses_behind);
        any_ahead = any_ahead || (occ && !uses_behind);
      }
      if (any_behind) {  // possible from the start of the stay on
        t_star = t_cur;
        e_star = e_cur;
        return true;
      }
      if (any_ahead) {
        t_star = fmaxf(t0, fminf(tm, t1));
        e_star = e_tie;
        return true;
      }
    }
    if (!(tm - em <= t1)) return false;  // the next crossing lies beyond the interval (or is NaN): the walk ends with it
    // Through a face of the box the walk does not step: t1 ends at that face's crossing taken e late (the slab test), and until then
    // the sample points may still be inside.  The axis stays in its last cell and the others go on.
    for (int a = 0; a < 3; ++a) {
      const int next = cell[a] + step[a];
      const bool leaves = next < 0 || next >= w.n[a];
      live[a] = live[a] && !(a == m && leaves);
      cell[a] = (a == m && !leaves) ? next : cell[a];
      t_prev[a] = (a == m && !leaves) ? tm : t_prev[a];
    }
    last = 1 << m;
    t_cur = fmaxf(t0, tm);
    e_cur = em;
  }
  return false;
}

__global__ void __launch_bounds__(RC_THREADS) rays_clip(const RcArgs s) {
  const int64_t r = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x;
  if (r >= s.rays.n_rays) return;
  const float near_t = s.rays.near_t[r], far_t = s.rays.far_t[r];  // (read before the stores below: the results may alias them)
  const int b = s.rays.grid_idx[r];
  RcWalk w;
  w.n[0] = s.W, w.n[1] = s.H, w.n[2] = s.D;
  bool ok = rc_finite(near_t) && rc_finite(far_t) && near_t <= far_t && b >= 0 && b < s.B;
  float dd = 0.0f;
  for (int a = 0; a < 3; ++a) {
    w.o[a] = s.rays.origins[r * 3 + a];
    w.d[a] = s.rays.directions[r * 3 + a];
    ok = ok && rc_finite(w.o[a]) && rc_finite(w.d[a]);
    dd = fmaf(w.d[a], w.d[a], dd);
  }
  // slab test; the cell of an axis that does not move is the Renderer's: rint of its un-normalised coordinate
  float t0 = near_t, t1 = far_t;
  int c[3] = {0, 0, 0};
  bool loose = false;  // a crossing this arithmetic cannot bound: the ray keeps its span
  for (int a = 0; a < 3; ++a) {
    w.moving[a] = w.d[a] != 0.0f;
    w.e[a] = 0.0f;
    if (!ok) continue;
    if (!w.moving[a]) {
      const float f = rintf(unnormalize<false>(w.o[a], w.n[a]));
      ok = fabsf(w.o[a]) <= 1.0f && f >= 0.0f && f <= (float)(w.n[a] - 1);
      c[a] = ok ? (int)f : 0;
      continue;
    }
    w.e[a] = RC_EPS * ((1.0f + fabsf(w.o[a])) / fabsf(w.d[a]));
    const float ta = (-1.0f - w.o[a]) / w.d[a], tb = (1.0f - w.o[a]) / w.d[a];
    if (!rc_finite(w.e[a]) || !rc_finite(ta) || !rc_finite(tb)) {
      loose = true;
      continue;
    }
    t0 = fmaxf(t0, fminf(ta, tb) - w.e[a]);
    t1 = fminf(t1, fmaxf(ta, tb) + w.e[a]);
  }
  ok = ok && t0 <= t1;
  float near_o = near_t, far_o = far_t;
  bool hit = ok;
  if (ok && !loose && (w.moving[0] || w.moving[1] || w.moving[2])) {
    float lo = t0, hi = t1, e_lo = 0.0f, e_hi = 0.0f;  // (the box's own e is already in t0 / t1)
    float h = 2.0f;
    if (s.scaffold) {
      const int nmax = max(s.W, max(s.H, s.D));
      h = 2.0f / (float)nmax;
      w.scaffold = s.scaffold + (int64_t)b * s.D * s.H * s.W;
      hit = rc_walk(w, t0, t1, c, lo, e_lo);
      if (hit) {
        RcWalk back = w;
        for (int a = 0; a < 3; ++a) back.d[a] = -w.d[a];
        float m = 0.0f;
        if (rc_walk(back, -t1, -t0, c, m, e_hi)) hi = -m;
        else hi = t1, e_hi = 0.0f;
      }
    }
    if (hit) {
      const float pad_t = s.pad * h / sqrtf(dd);
      near_o = fmaxf(near_t, lo - pad_t - e_lo);
      far_o = fminf(far_t, hi + pad_t + e_hi);
      far_o = fmaxf(far_o, near_o);
    }
  } else if (ok && !loose && s.scaffold) {  // d == 0: the ray is one point, in one cell
    w.scaffold = s.scaffold + (int64_t)b * s.D * s.H * s.W;
    hit = rc_occupied(w, c[0], c[1], c[2]);
  }
  s.near_out[r] = near_o;
  s.far_out[r] = far_o;
  s.hit_out[r] = hit ? 1 : 0;
}

// `a` checked by lp_api.hip
int rays_clip_launch(const LpRayClipArgs& a, float* near_out, float* far_out, uint8_t* hit_out, hipStream_t stream) {
  RcArgs s;
  s.rays = a.rays;
  s.scaffold = a.scaffold;
  s.B = a.scaffold ? a.scaffold_shape.B : 0x7fffffff;  // (box only: one scene, any grid_idx >= 0)
  s.D = a.scaffold ? a.scaffold_shape.D : 1;
  s.H = a.scaffold ? a.scaffold_shape.H : 1;
  s.W = a.scaffold ? a.scaffold_shape.W : 1;
  s.pad = a.pad;
  s.near_out = near_out, s.far_out = far_out, s.hit_out = hit_out;
  unsigned blocks;
  if (int rc = launch_blocks("lp_rays_clip", a.rays.n_rays, RC_THREADS, blocks)) return rc;
  hipLaunchKernelGGL(rays_clip, dim3(blocks), dim3(RC_THREADS), 0, stream, s);
  return check_launch("rays_clip");
}

const char* build_info_ray_clip() {
  return "{\"walk\": \"one lane per ray, one wave per workgroup; 3-D DDA over the scaffold's cells, forward to the first occupied cell and "
         "backward from the far end; crossings from plane indices (no accumulation); integer-bounded loops; no atomics, no workspace\"}";
}

}  // namespace lp

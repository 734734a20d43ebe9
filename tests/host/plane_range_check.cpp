// plane_range_check.cpp -- stand-alone host check of lp_plane_range.h (the per-wave sample ranges of the tuned Renderer kernels).
//
//   plane_range_check RAYS.bin
//
// RAYS.bin: int32 n_rays, S, W, H, D; then float32 origins[3 n], directions[3 n], near[n], far[n] (tests/test_plane_range_host.py
// writes it).  For every wave (32 consecutive rays) the ranges are formed exactly as the kernels form them -- ray_axis_spans(),
// plane_span() / voxel_span(), hull over the wave's rays -- and every (ray, sample, grid) is then evaluated by brute force with the
// march's own float arithmetic (lin01, sample_point, unnormalize, axis_taps of lp_device.h, restated below; build with
// -ffp-contract=off).  A tap of non-zero weight at a sample outside the wave's range is a violation.  Prints one JSON line:
// violations, and the fraction of (wave, sample, grid) triples the ranges leave out next to the fraction that is really empty.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../lightplane_amd/csrc/lp_plane_range.h"

namespace {

float lin01(int i, int S) {
  if (S <= 1) return 0.0f;
  const float step = 1.0f / (float)(S - 1);
  return (i < S / 2) ? step * (float)i : 1.0f - step * (float)(S - 1 - i);
}

// any tap of this axis in range with non-zero weight
struct Axis {
  bool ok[2];
  float w[2];
};
Axis axis_taps(float c, int size) {
  const float t = ((c + 1.0f) * (float)size - 1.0f) / 2.0f;
  const float f = floorf(t);
  const int i0 = (int)fminf(fmaxf(f, -2.0f), (float)size);
  Axis a;
  a.w[1] = t - f;
  a.w[0] = (f + 1.0f) - t;
  a.ok[0] = (unsigned)i0 < (unsigned)size;
  a.ok[1] = (unsigned)(i0 + 1) < (unsigned)size;
  return a;
}
bool plane_live(const Axis& u, const Axis& v) {
  for (int k = 0; k < 4; ++k)
    if (u.ok[k & 1] && v.ok[k >> 1] && u.w[k & 1] * v.w[k >> 1] != 0.0f) return true;
  return false;
}
bool voxel_live(const Axis& x, const Axis& y, const Axis& z) {
  for (int k = 0; k < 8; ++k)
    if (x.ok[k & 1] && y.ok[(k >> 1) & 1] && z.ok[k >> 2] && (x.w[k & 1] * y.w[(k >> 1) & 1]) * z.w[k >> 2] != 0.0f) return true;
  return false;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s RAYS.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int32_t hdr[5];
  if (fread(hdr, sizeof(int32_t), 5, f) != 5) { fprintf(stderr, "short header\n"); return 2; }
  const int n = hdr[0], S = hdr[1], W = hdr[2], H = hdr[3], D = hdr[4];
  if (n <= 0 || S <= 0 || W < 2 || H < 2 || D < 2) { fprintf(stderr, "bad header\n"); return 2; }
  std::vector<float> org(3 * (size_t)n), dir(3 * (size_t)n), nr(n), fr(n);
  if (fread(org.data(), 4, org.size(), f) != org.size() || fread(dir.data(), 4, dir.size(), f) != dir.size() ||
      fread(nr.data(), 4, nr.size(), f) != nr.size() || fread(fr.data(), 4, fr.size(), f) != fr.size()) {
    fprintf(stderr, "short body\n");
    return 2;
  }
  fclose(f);

  // grid 0..2: the planes of the triplane, 3: the voxel grid
  long long triples = 0, skipped[4] = {0, 0, 0, 0}, empty[4] = {0, 0, 0, 0}, violations = 0, all_skipped = 0;
  std::vector<unsigned char> live((size_t)S * 4);
  for (int r0 = 0; r0 < n; r0 += 32) {
    const int r1 = r0 + 32 < n ? r0 + 32 : n;
    lp::SampleSpan hull[4] = {lp::span_none(S), lp::span_none(S), lp::span_none(S), lp::span_none(S)};
    for (int r = r0; r < r1; ++r) {
      const lp::AxisSpans ax = lp::ray_axis_spans(org[3 * r], org[3 * r + 1], org[3 * r + 2], dir[3 * r], dir[3 * r + 1], dir[3 * r + 2],
                                                  nr[r], fr[r], S, W, H, D);
      for (int g = 0; g < 3; ++g) hull[g] = lp::span_hull(hull[g], lp::plane_span(ax, g, S));
      hull[3] = lp::span_hull(hull[3], lp::voxel_span(ax, S));
    }
    if (r1 - r0 < 32)  // a wave with invalid lanes keeps every sample (as the kernels do)
      for (int g = 0; g < 4; ++g) hull[g] = lp::span_full(S);
    for (size_t i = 0; i < live.size(); ++i) live[i] = 0;
    for (int r = r0; r < r1; ++r) {
      for (int s = 0; s < S; ++s) {
        const float depth = nr[r] + lin01(s, S) * (fr[r] - nr[r]);
        const float x = depth * dir[3 * r] + org[3 * r], y = depth * dir[3 * r + 1] + org[3 * r + 1], z = depth * dir[3 * r + 2] + org[3 * r + 2];
        const Axis ax = axis_taps(x, W), ay = axis_taps(y, H), az = axis_taps(z, D);
        const bool lv[4] = {plane_live(ax, ay), plane_live(ax, az), plane_live(ay, az), voxel_live(ax, ay, az)};
        for (int g = 0; g < 4; ++g) {
          if (!lv[g]) continue;
          live[(size_t)s * 4 + g] = 1;
          if (s < hull[g].lo || s > hull[g].hi) {
            if (violations < 10)
              fprintf(stderr, "violation: ray %d sample %d grid %d live outside [%d, %d]\n", r, s, g, hull[g].lo, hull[g].hi);
            ++violations;
          }
        }
      }
    }
    for (int s = 0; s < S; ++s) {
      ++triples;
      bool all = true;
      for (int g = 0; g < 4; ++g) {
        const bool out = s < hull[g].lo || s > hull[g].hi;
        skipped[g] += out;
        empty[g] += !live[(size_t)s * 4 + g];
        if (g < 3) all = all && out;
      }
      all_skipped += all;
    }
  }
  const double t3 = 3.0 * (double)triples;
  printf("{\"n_rays\": %d, \"S\": %d, \"violations\": %lld, \"triplane_skipped\": %.4f, \"triplane_empty\": %.4f, "
         "\"triplane_all_planes_skipped\": %.4f, \"plane_skipped\": [%.4f, %.4f, %.4f], \"voxel_skipped\": %.4f, \"voxel_empty\": %.4f}\n",
         n, S, violations, (double)(skipped[0] + skipped[1] + skipped[2]) / t3, (double)(empty[0] + empty[1] + empty[2]) / t3,
         (double)all_skipped / (double)triples, (double)skipped[0] / (double)triples, (double)skipped[1] / (double)triples,
         (double)skipped[2] / (double)triples, (double)skipped[3] / (double)triples, (double)empty[3] / (double)triples);
  return violations ? 1 : 0;
}

#!/usr/bin/env python
"""Developer benchmark of the weighted splat / gather along rays (lightplane_amd/ray_grid.py) on one MI355X.

    python scripts/bench_ray_grid.py [--reps 10] [--warmup 2] [--out profiles/ray_grid_bench.txt]

Times five operations two ways in ONE process, alternating:
  chain   the composition the library offered before: the points o + t d and the expanded [R, S, C] tensor W[..., None] * F[:, None]
          through lp.splat_points(normalize=False), resp. (lp.sample_grid_at_points(...) * W[..., None]).sum(1); for unit weights
          lp.lightplane_splatter on the same rays
  fused   lp.splat_along_rays / lp.gather_along_rays
for 65 536 and 4 096 rays x 128 samples (the depths of lp.ray_samples, random weights in [0, 1)), random rays and the rays of a
pinhole image, on a 128^2 x 32 triplane and a 128^3 x 32 voxel grid:
  splat forward           the per-ray features lifted into a zeroed grid-list (no_grad)
  splat fwd+bwd           ... and the gradient of <result, G> into the features and the weights
  gather forward          the grids rendered with the weights (no_grad)
  gather fwd+bwd          ... and the gradient of <result, U> into the grids and the weights
  unit splat (norm.)      weights = 1, normalised, against lp.lightplane_splatter (forward)
Times are device-event medians over --reps calls after --warmup calls, two passes per path; memory is
torch.cuda.max_memory_allocated above what was allocated before the calls (results and gradients included).  The splat rows also give
the fraction reached of the chip-wide float-atomic rate (~1.3 TB/s of added bytes, samples x corners x C x 4 bytes).
Every workload runs in a child process of its own under a time limit, one after the other, and the script stops at the first that
fails.  It needs a GPU and fails without one.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lightplane_amd as lp  # noqa: E402
from lightplane_amd import _lib  # noqa: E402
from tests.synth import pinhole_rays, random_rays  # noqa: E402

GRIDS = {
    "triplane_128^2x32": [(1, 1, 128, 128, 32), (1, 128, 1, 128, 32), (1, 128, 128, 1, 32)],
    "voxel_128^3x32": [(1, 128, 128, 128, 32)],
}
RAYS = {"65536": 256, "4096": 64}  # rays: side of the pinhole image
KINDS = ("random", "pinhole")
S = 128
ATOMIC_BYTES_PER_S = 1.3e12
STEP_LIMIT_S = 240  # per workload (a child process): many times what the slowest one is expected to take


def timed(fn, reps, warmup):
    """(median ms, min ms, max ms, peak bytes above the starting allocation) of fn()"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms), torch.cuda.max_memory_allocated() - base


def workload(gname, rname, kind, reps, warmup):
    dev = torch.device("cuda:0")
    sizes = [list(s) for s in GRIDS[gname]]
    C = sizes[0][4]
    gen = torch.Generator().manual_seed(0)
    side = RAYS[rname]
    rays = (random_rays(gen, side * side, 1, C) if kind == "random" else pinhole_rays(side, side, enc_dim=C, gen=gen)).to(dev)
    R = rays.directions.shape[0]
    dgen = torch.Generator(device=dev).manual_seed(1)
    grids = [(0.5 * torch.randn(*s, device=dev, generator=dgen)).requires_grad_(True) for s in sizes]
    ups = [torch.randn(*s, device=dev, generator=dgen) for s in sizes]
    t = lp.ray_samples(rays, S).depths.contiguous()
    o, d, idx = rays.origins, rays.directions, rays.grid_idx
    w = torch.rand(R, S, device=dev, generator=dgen).requires_grad_(True)
    f = rays.encoding.clone().requires_grad_(True)
    g_out = torch.randn(R, C, device=dev, generator=dgen)
    ones = torch.ones(R, S, device=dev)

    def chain_splat(ww, ff):
        pts = t[..., None] * d[:, None, :] + o[:, None, :]
        return lp.splat_points(pts, (ww[..., None] * ff[:, None, :]).contiguous(), sizes, idx, normalize=False)

    def chain_gather(ww):
        pts = t[..., None] * d[:, None, :] + o[:, None, :]
        return (lp.sample_grid_at_points(pts, grids, idx) * ww[..., None]).sum(1)

    def splat_forward(fused):
        with torch.no_grad():
            return lp.splat_along_rays(rays, t, w, f, sizes) if fused else chain_splat(w, f)

    def splat_fwd_bwd(fused):
        w.grad = f.grad = None
        outs = lp.splat_along_rays(rays, t, w, f, sizes) if fused else chain_splat(w, f)
        sum((x * u).sum() for x, u in zip(outs, ups)).backward()
        return [x.detach() for x in outs] + [f.grad, w.grad]

    def gather_forward(fused):
        with torch.no_grad():
            return lp.gather_along_rays(rays, t, w, grids) if fused else chain_gather(w)

    def gather_fwd_bwd(fused):
        w.grad = None
        for g in grids:
            g.grad = None
        out = lp.gather_along_rays(rays, t, w, grids) if fused else chain_gather(w)
        (out * g_out).sum().backward()
        return [out.detach(), w.grad] + [g.grad for g in grids]

    def unit_splat(fused):
        with torch.no_grad():
            if fused:
                return lp.splat_along_rays(rays, t, ones, f, sizes, normalize=True)
            return lp.lightplane_splatter(rays, sizes, num_samples=S)

    corners = sum(8 if min(s[1:4]) > 1 else 4 for s in sizes)
    floor_ms = R * S * corners * C * 4 / ATOMIC_BYTES_PER_S * 1e3
    lines = [f"\n{gname}, {R} {kind} rays x {S} samples; atomic floor of one splat {floor_ms:.3f} ms ({corners} corner rows per sample)"]
    rows = {}
    ops = (("splat forward", splat_forward, 1), ("splat fwd+bwd", splat_fwd_bwd, 1), ("gather forward", gather_forward, 0),
           ("gather fwd+bwd", gather_fwd_bwd, 1), ("unit splat (norm.)", unit_splat, 1))
    for what, fn, splats in ops:
        res = {}
        for key, fused in (("chain", False), ("fused", True), ("chain", False), ("fused", True)):
            res.setdefault(key, []).append(timed(lambda: fn(fused), reps, warmup))
        for key in ("chain", "fused"):
            for i, r in enumerate(res[key]):
                lines.append(f"  {what:18s} {key:6s} pass {i}: {r[0]:9.3f} ms [{r[1]:.3f} .. {r[2]:.3f}]  mem +{r[3] / 2 ** 20:9.1f} MiB")
        tc, tf = (statistics.median(r[0] for r in res[k]) for k in ("chain", "fused"))
        mc, mf = (max(r[3] for r in res[k]) for k in ("chain", "fused"))
        spread = max(abs(res[k][0][0] - res[k][1][0]) for k in ("chain", "fused"))
        rows[what] = (tc, tf, mc, mf, spread)
        frac = f"; one splat's atomic floor is {floor_ms / tf:.2f} of the fused time" if splats else ""
        lines.append(f"  {what:18s} chain / fused: time {tc / tf:.2f} x ({tc:.3f} -> {tf:.3f} ms, spread between passes {spread:.3f} ms), "
                     f"memory {mc / 2 ** 20:.1f} -> {mf / 2 ** 20:.1f} MiB{frac}")
        a, b = fn(False), fn(True)
        a, b = (a, b) if isinstance(a, (list, tuple)) else ([a], [b])
        worst = max(float((x - y).abs().max()) / max(float(x.abs().max()), 1e-30) for x, y in zip(a, b))
        lines.append(f"  {what:18s} the two paths differ by at most {worst:.2e} of a result's max |value|")
    return lines, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help="(internal) run one workload 'grids|rays|kind' and print its JSON report")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ray_grid.py measures on a GPU; there is nothing to fall back to"
    if a.one:
        lines, rows = workload(*a.one.split("|"), a.reps, a.warmup)
        print("__REPORT__" + json.dumps({"lines": lines, "rows": rows}), flush=True)
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# ray-grid bench  {time.strftime('%Y-%m-%d')}  {torch.cuda.get_device_name(0)}  library src {_lib.build_info()['src_hash'][:16]}")
    say(f"# lp.splat_along_rays / lp.gather_along_rays against the composition through [R, S, C] tensors (lp.splat_points / "
        f"lp.sample_grid_at_points; unit weights: lp.lightplane_splatter); median of {a.reps} calls after {a.warmup} warm-up calls "
        "(device events), the two paths alternating, two passes each; min / max in brackets; mem = peak bytes above the start")
    slower = []
    for gname in GRIDS:
        for rname in RAYS:
            for kind in KINDS:
                cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps),
                       "--warmup", str(a.warmup), "--one", f"{gname}|{rname}|{kind}"]
                p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                rep = [ln for ln in p.stdout.splitlines() if ln.startswith("__REPORT__")]
                if p.returncode != 0 or not rep:
                    say(f"\n{gname}, {rname} {kind} rays: FAILED (exit status {p.returncode}); nothing more is run\n{p.stdout[-2000:]}")
                    sys.exit(1)
                r = json.loads(rep[0][len("__REPORT__"):])
                for ln in r["lines"]:
                    say(ln)
                for what, (tc, tf, _, _, spread) in r["rows"].items():
                    if tf > tc + spread:
                        slower.append(f"{gname} {rname} {kind} {what}: {tc:.3f} -> {tf:.3f} ms")
    say("\n# rows where the fused path is slower than the composition beyond the spread between passes: "
        + ("none" if not slower else "; ".join(slower)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Developer benchmark of the gather / splat of a grid-list at points (lightplane_amd/point_grid.py) on one MI355X.

    python scripts/bench_point_grid.py [--reps 10] [--warmup 2] [--out profiles/point_grid_bench.txt]

Times four operations two ways in ONE process, alternating:
  torch   the PyTorch composition: every grid permuted to channels-first, ``F.grid_sample(align_corners=False, padding_mode="zeros")``
          per grid entry (5-D for a voxel grid, 4-D on the two live axes for a plane), summed; its autograd for the scatter
  fused   lp.sample_grid_at_points / lp.splat_points
for 2^18 and 2^20 random points in [-1.2, 1.2]^3 (512 resp. 1 024 rows of 512 resp. 1 024 points) on a 128^2 x 32 triplane and a
128^3 x 32 voxel grid:
  gather forward          features at the points (no_grad)
  gather fwd+bwd          ... and the gradient of <features, U> into the grids
  raw splat               the features lifted into a zeroed grid-list (torch: the autograd adjoint of its gather)
  normalised splat f+b    F / clamp(W, 1e-5) with W the splat of ones, and the gradient of <result, G> into the features (torch: the
                          adjoint for F and for W, then the gather of G / clamp(W))
Times are device-event medians over --reps calls after --warmup calls, two passes per path; memory is
torch.cuda.max_memory_allocated above what was allocated before the calls (results and gradients included).  The splat rows also give
the fraction reached of the chip-wide float-atomic rate (~1.3 TB/s of added bytes: points x corners x C x 4 bytes).  Every workload
runs in a child process of its own under a time limit, one after the other, and the script stops at the first that fails.  It needs a
GPU and fails without one.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lightplane_amd as lp  # noqa: E402
from lightplane_amd import _lib  # noqa: E402

GRIDS = {
    "triplane_128^2x32": [(1, 1, 128, 128, 32), (1, 128, 1, 128, 32), (1, 128, 128, 1, 32)],
    "voxel_128^3x32": [(1, 128, 128, 128, 32)],
}
POINTS = {"2^18": (512, 512), "2^20": (1024, 1024)}
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


def torch_gather(grids, pts):
    """sum over the list of grid_sample at pts [P, 3]; every grid has B == 1"""
    out = None
    for g in grids:
        _, D, H, W, C = g.shape
        if D > 1 and H > 1 and W > 1:
            s = F.grid_sample(g.permute(0, 4, 1, 2, 3), pts.view(1, 1, 1, -1, 3), mode="bilinear", padding_mode="zeros", align_corners=False)
            s = s.view(C, -1)
        else:
            if D == 1:
                img, uv = g[:, 0], pts[:, [0, 1]]
            elif H == 1:
                img, uv = g[:, :, 0], pts[:, [0, 2]]
            else:
                img, uv = g[:, :, :, 0], pts[:, [1, 2]]
            s = F.grid_sample(img.permute(0, 3, 1, 2), uv.reshape(1, 1, -1, 2), mode="bilinear", padding_mode="zeros", align_corners=False)
            s = s.view(C, -1)
        out = s if out is None else out + s
    return out.t()


def torch_splat(sizes, pts, feat, dev):
    """the adjoint of torch_gather by autograd: a list of [1, D, H, W, C]"""
    zeros = [torch.zeros(*s[:4], feat.shape[-1], device=dev, requires_grad=True) for s in sizes]
    (torch_gather(zeros, pts) * feat).sum().backward()
    return [z.grad for z in zeros]


def workload(gname, pname, reps, warmup):
    dev = torch.device("cuda:0")
    sizes = GRIDS[gname]
    R, N = POINTS[pname]
    C = sizes[0][4]
    gen = torch.Generator(device=dev).manual_seed(0)
    grids = [(0.5 * torch.randn(*s, device=dev, generator=gen)).requires_grad_(True) for s in sizes]
    ups = [torch.randn(*s, device=dev, generator=gen) for s in sizes]
    pts = torch.rand(R, N, 3, device=dev, generator=gen) * 2.4 - 1.2
    flat_pts = pts.view(-1, 3)
    idx = torch.zeros(R, dtype=torch.long, device=dev)
    vec = torch.randn(R, N, C, device=dev, generator=gen)
    flat_vec = vec.view(-1, C)
    feat = vec.clone().requires_grad_(True)
    ones = torch.ones(R * N, 1, device=dev)

    def gather_forward(fused):
        with torch.no_grad():
            return lp.sample_grid_at_points(pts, grids, idx) if fused else torch_gather(grids, flat_pts).view(R, N, C)

    def gather_fwd_bwd(fused):
        for g in grids:
            g.grad = None
        out = lp.sample_grid_at_points(pts, grids, idx) if fused else torch_gather(grids, flat_pts).view(R, N, C)
        (out * vec).sum().backward()
        return [g.grad for g in grids]

    def raw_splat(fused):
        if fused:
            with torch.no_grad():
                return lp.splat_points(pts, vec, sizes, idx, normalize=False)
        return torch_splat(sizes, flat_pts, flat_vec, dev)

    def norm_splat_fwd_bwd(fused):
        feat.grad = None
        if fused:
            outs = lp.splat_points(pts, feat, sizes, idx, normalize=True)
            sum((o * u).sum() for o, u in zip(outs, ups)).backward()
            return [o.detach() for o in outs] + [feat.grad]
        fsum = torch_splat(sizes, flat_pts, flat_vec, dev)
        wsum = [w.clamp(min=1e-5) for w in torch_splat(sizes, flat_pts, ones, dev)]
        outs = [f / w for f, w in zip(fsum, wsum)]
        with torch.no_grad():
            d_feat = torch_gather([u / w for u, w in zip(ups, wsum)], flat_pts).view(R, N, C)
        return outs + [d_feat]

    corners = sum(8 if min(s[1:4]) > 1 else 4 for s in sizes)
    floor_ms = R * N * corners * C * 4 / ATOMIC_BYTES_PER_S * 1e3
    lines = [f"\n{gname}, {pname} points ({R} rows x {N}); atomic floor of one splat {floor_ms:.3f} ms ({corners} corner rows per point)"]
    rows = {}
    ops = (("gather forward", gather_forward, 0), ("gather fwd+bwd", gather_fwd_bwd, 1), ("raw splat", raw_splat, 1),
           ("norm. splat f+b", norm_splat_fwd_bwd, 1))
    for what, fn, splats in ops:
        res = {}
        for key, fused in (("torch", False), ("fused", True), ("torch", False), ("fused", True)):
            res.setdefault(key, []).append(timed(lambda: fn(fused), reps, warmup))
        for key in ("torch", "fused"):
            for i, r in enumerate(res[key]):
                lines.append(f"  {what:16s} {key:6s} pass {i}: {r[0]:9.3f} ms [{r[1]:.3f} .. {r[2]:.3f}]  mem +{r[3] / 2 ** 20:9.1f} MiB")
        tt, tf = (statistics.median(r[0] for r in res[k]) for k in ("torch", "fused"))
        mt, mf = (max(r[3] for r in res[k]) for k in ("torch", "fused"))
        rows[what] = (tt, tf, mt, mf)
        frac = f"; one splat's atomic floor is {floor_ms / tf:.2f} of the fused time" if splats else ""
        lines.append(f"  {what:16s} torch / fused: time {tt / tf:.2f} x ({tt:.3f} -> {tf:.3f} ms), memory {mt / max(mf, 1):.1f} x; "
                     f"fused {tf * 1e6 / (R * N):.2f} ns per point{frac}")
        a, b = fn(False), fn(True)
        a, b = (a, b) if isinstance(a, (list, tuple)) else ([a], [b])
        worst = max(float((x - y).abs().max()) / max(float(x.abs().max()), 1e-30) for x, y in zip(a, b))
        lines.append(f"  {what:16s} the two paths differ by at most {worst:.2e} of a result's max |value|")
    return lines, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help="(internal) run one workload 'scene|points' and print its JSON report")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_point_grid.py measures on a GPU; there is nothing to fall back to"
    if a.one:
        lines, rows = workload(*a.one.split("|"), a.reps, a.warmup)
        print("__REPORT__" + json.dumps({"lines": lines, "rows": rows}), flush=True)
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# point-grid bench  {time.strftime('%Y-%m-%d')}  {torch.cuda.get_device_name(0)}  library src {_lib.build_info()['src_hash'][:16]}")
    say(f"# lp.sample_grid_at_points / lp.splat_points against permute + F.grid_sample per grid + sum (and its autograd); median of "
        f"{a.reps} calls after {a.warmup} warm-up calls (device events), the two paths alternating, two passes each; min / max in "
        "brackets; mem = peak bytes above the start")
    slower = []
    for gname in GRIDS:
        for pname in POINTS:
            cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps),
                   "--warmup", str(a.warmup), "--one", f"{gname}|{pname}"]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            rep = [ln for ln in p.stdout.splitlines() if ln.startswith("__REPORT__")]
            if p.returncode != 0 or not rep:
                say(f"\n{gname}, {pname}: FAILED (exit status {p.returncode}); nothing more is run\n{p.stdout[-2000:]}")
                sys.exit(1)
            r = json.loads(rep[0][len("__REPORT__"):])
            for ln in r["lines"]:
                say(ln)
            for what, (tt, tf, _, _) in r["rows"].items():
                if tf > tt:
                    slower.append(f"{gname} {pname} {what}: {tt:.3f} -> {tf:.3f} ms")
    say("\n# rows where the fused path is slower than the PyTorch composition: " + ("none" if not slower else "; ".join(slower)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Developer benchmark of the decoder evaluation at points (lightplane_amd/points.py) on one MI355X.

    python scripts/bench_points.py [--reps 10] [--warmup 2] [--out profiles/points_bench.txt]

Times ``LightplaneRenderer.eval_decoder_at_points`` two ways in ONE process, alternating:
  renderer   config.fused_module_ops = False: two single-sample renders (the second at gain 1e30 for the colour)
  fused      config.fused_module_ops = True: lp.lightplane_eval_mlp (one forward kernel; the backward recomputes the decoder)
for 2^18 and 2^20 random points in [-1.2, 1.2]^3 (512 resp. 1 024 rays of 512 resp. 1 024 points) on a 128^2 x 32 triplane and a
128^3 x 32 voxel grid, decoders 2/2/2 x 32 and 1/1/2 x 64: the forward alone (no_grad) and forward + backward of
``opacity.sum() + colour.sum()`` into the grids, the decoder's parameters and the encoding.  Times are device-event medians over --reps
calls after --warmup calls; memory is torch.cuda.max_memory_allocated above what was allocated before the calls (results and
gradients included).  Every workload runs in a child process of its own under a time limit, one after the other, and the script stops
at the first that fails.  It needs a GPU and fails without one.
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
from lightplane_amd import _lib, config  # noqa: E402

GRIDS = {
    "triplane_128^2x32": [(1, 1, 128, 128, 32), (1, 128, 1, 128, 32), (1, 128, 128, 1, 32)],
    "voxel_128^3x32": [(1, 128, 128, 128, 32)],
}
DECODERS = {"2/2/2x32": (2, 2, 2, 32), "1/1/2x64": (1, 1, 2, 64)}
POINTS = {"2^18": (512, 512), "2^20": (1024, 1024)}
STEP_LIMIT_S = 240  # per workload (a child process): about twenty times what the slowest one is expected to take


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


def workload(gname, dname, pname, reps, warmup):
    """one (scene, decoder, point count): four timings per path, alternating; returns the lines of its report"""
    dev = torch.device("cuda:0")
    n_t, n_o, n_c, hidden = DECODERS[dname]
    R, N = POINTS[pname]
    torch.manual_seed(0)
    mod = lp.LightplaneRenderer(num_samples=128, color_chn=3, grid_chn=32, mlp_hidden_chn=hidden, mlp_n_layers_trunk=n_t,
                                mlp_n_layers_opacity=n_o, mlp_n_layers_color=n_c, opacity_init_bias=-1.0,
                                ray_embedding_num_harmonics=None).to(dev)
    with torch.no_grad():
        mod.mlp_params.mul_(3.0)
    gen = torch.Generator(device=dev).manual_seed(0)
    grids = [(0.5 * torch.randn(*s, device=dev, generator=gen)).requires_grad_(True) for s in GRIDS[gname]]
    pts = torch.rand(R, N, 3, device=dev, generator=gen) * 2.4 - 1.2
    idx = torch.zeros(R, dtype=torch.long, device=dev)
    enc = torch.randn(R, mod.rays_encoding_dim, device=dev, generator=gen).requires_grad_(True)

    def forward(fused):
        config.fused_module_ops = fused
        try:
            with torch.no_grad():
                return mod.eval_decoder_at_points(pts, idx, enc, grids)
        finally:
            config.fused_module_ops = True

    def forward_backward(fused):
        config.fused_module_ops = fused
        try:
            for t in grids + [enc, mod.mlp_params]:
                t.grad = None
            op, col = mod.eval_decoder_at_points(pts, idx, enc, grids)
            (op.sum() + col.sum()).backward()
        finally:
            config.fused_module_ops = True

    lines = [f"\n{gname}, decoder {dname}, {pname} points ({R} rays x {N})"]
    rows = {}
    for what, fn in (("forward", forward), ("fwd+bwd", forward_backward)):
        res = {}
        for key, fused in (("renderer", False), ("fused", True), ("renderer", False), ("fused", True)):
            res.setdefault(key, []).append(timed(lambda: fn(fused), reps, warmup))
        for key in ("renderer", "fused"):
            for i, r in enumerate(res[key]):
                lines.append(f"  {what:8s} {key:8s} pass {i}: {r[0]:9.3f} ms [{r[1]:.3f} .. {r[2]:.3f}]  mem +{r[3] / 2 ** 20:9.1f} MiB")
        tr, tf = (statistics.median(r[0] for r in res[k]) for k in ("renderer", "fused"))
        mr, mf = (max(r[3] for r in res[k]) for k in ("renderer", "fused"))
        rows[what] = (tr, tf, mr, mf)
        lines.append(f"  {what:8s} renderer / fused: time {tr / tf:.2f} x ({tr:.3f} -> {tf:.3f} ms), memory {mr / max(mf, 1):.1f} x; "
                     f"fused {tf * 1e6 / (R * N):.2f} ns per point")
    a, b = forward(False), forward(True)
    scale = [float(x.abs().max()) for x in a]
    lines.append("  the two paths differ by at most " + ", ".join(f"{float((x - y).abs().max()) / s:.2e}" for x, y, s in zip(a, b, scale))
                 + " of max |opacity|, max |colour|")
    return lines, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help="(internal) run one workload 'scene|decoder|points' and print its JSON report")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_points.py measures on a GPU; there is nothing to fall back to"
    if a.one:
        lines, rows = workload(*a.one.split("|"), a.reps, a.warmup)
        print("__REPORT__" + json.dumps({"lines": lines, "rows": rows}), flush=True)
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# points bench  {time.strftime('%Y-%m-%d')}  {torch.cuda.get_device_name(0)}  library src {_lib.build_info()['src_hash'][:16]}")
    say(f"# LightplaneRenderer.eval_decoder_at_points; median of {a.reps} calls after {a.warmup} warm-up calls (device events), the two "
        "paths alternating per workload; min / max in brackets; mem = peak bytes above the start")
    slower = []
    for gname in GRIDS:
        for dname in DECODERS:
            for pname in POINTS:
                cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps),
                       "--warmup", str(a.warmup), "--one", f"{gname}|{dname}|{pname}"]
                p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                rep = [ln for ln in p.stdout.splitlines() if ln.startswith("__REPORT__")]
                if p.returncode != 0 or not rep:
                    say(f"\n{gname}, decoder {dname}, {pname}: FAILED (exit status {p.returncode}); nothing more is run\n{p.stdout[-2000:]}")
                    sys.exit(1)
                r = json.loads(rep[0][len("__REPORT__"):])
                for ln in r["lines"]:
                    say(ln)
                for what, (tr, tf, _, _) in r["rows"].items():
                    if tf > tr:
                        slower.append(f"{gname} {dname} {pname} {what}: {tr:.3f} -> {tf:.3f} ms")
    say("\n# rows where the fused path is slower than the Renderer path: " + ("none" if not slower else "; ".join(slower)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

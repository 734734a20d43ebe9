#!/usr/bin/env python
"""Developer benchmark of the occupancy scaffold (lightplane_amd/scaffold.py) on one MI355X.

    python scripts/bench_scaffold.py [--reps 10] [--warmup 2] [--out profiles/scaffold_bench.txt]

Times ``LightplaneRenderer.calculate_scaffold`` (decoder 2/2/2 x 32, dilate_scaffold 2) two ways in ONE process, alternating:
  renderer   config.fused_module_ops = False: the lattice as single-sample rays through the Renderer, max_pool3d on the float lattice
  fused      config.fused_module_ops = True: lp.calculate_scaffold (one lattice kernel + three byte passes)
for scaffolds of 128^3 and 256^3 points on a 128^2 x 32 triplane and a 128^3 x 32 voxel grid.  Times are device-event medians over
--reps calls after --warmup calls; memory is torch.cuda.max_memory_allocated above what was allocated before the calls (the result
included).  The two scaffolds are compared at the median opacity, where fp32 round-off may flip single points: the share of points that
differ is printed, not asserted (the tests hold both paths to the oracle).  The script needs a GPU and fails without one.
"""
import argparse
import os
import statistics
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
SCAFFOLDS = (128, 256)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default=",".join(str(s) for s in SCAFFOLDS), help="comma-separated scaffold edge lengths")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_scaffold.py measures on a GPU; there is nothing to fall back to"
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# scaffold bench  {time.strftime('%Y-%m-%d')}  {torch.cuda.get_device_name(0)}  library src {_lib.build_info()['src_hash'][:16]}")
    say(f"# LightplaneRenderer.calculate_scaffold, decoder 2/2/2 x 32, dilate_scaffold 2; median of {a.reps} calls after {a.warmup} warm-up "
        "calls (device events), the two paths alternating per workload; min / max in brackets; mem = peak bytes above the start")
    torch.manual_seed(0)
    mod = lp.LightplaneRenderer(num_samples=128, color_chn=3, grid_chn=32, mlp_hidden_chn=32, opacity_init_bias=-1.0,
                                ray_embedding_num_harmonics=None).to(dev)
    with torch.no_grad():
        mod.mlp_params.mul_(3.0)
    for gname, shapes in GRIDS.items():
        gen = torch.Generator(device=dev).manual_seed(0)
        grids = [0.5 * torch.randn(*s, device=dev, generator=gen) for s in shapes]
        for n in (int(v) for v in a.sizes.split(",")):
            size = [1, n, n, n]
            t = float(lp.scaffold_opacity(grids, mod.get_decoder_params(), size, gain=mod.gain).median())
            say(f"\n{gname}, scaffold {n}^3 ({4 * n ** 3 / 2 ** 20:.0f} MiB result), threshold {t:.4g} (the median opacity)")

            def run(fused):
                config.fused_module_ops = fused
                try:
                    return mod.calculate_scaffold(grids, size, dev, threshold=t)
                finally:
                    config.fused_module_ops = True

            res, outs = {}, {}
            for key, fused in (("renderer", False), ("fused", True), ("renderer", False), ("fused", True)):
                try:
                    r = timed(lambda: run(fused), a.reps, a.warmup)
                    outs[key] = run(fused)
                except torch.cuda.OutOfMemoryError:
                    r = None
                    torch.cuda.empty_cache()
                res.setdefault(key, []).append(r)
            for key in ("renderer", "fused"):
                for i, r in enumerate(res[key]):
                    if r is None:
                        say(f"  {key:8s} pass {i}: does not fit (out of memory)")
                    else:
                        say(f"  {key:8s} pass {i}: {r[0]:9.3f} ms [{r[1]:.3f} .. {r[2]:.3f}]  mem +{r[3] / 2 ** 20:9.1f} MiB")
            ok = [k for k in ("renderer", "fused") if all(r is not None for r in res[k])]
            if len(ok) == 2:
                tr = statistics.median(r[0] for r in res["renderer"])
                tf = statistics.median(r[0] for r in res["fused"])
                mr, mf = max(r[3] for r in res["renderer"]), max(r[3] for r in res["fused"])
                diff = float((outs["renderer"] != outs["fused"]).float().mean())
                say(f"  renderer / fused: time {tr / tf:.2f} x, memory {mr / mf:.1f} x; occupied {float(outs['fused'].mean()):.3f}; "
                    f"points that differ between the paths: {diff:.2e}")
            del outs
            torch.cuda.empty_cache()
        del grids
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

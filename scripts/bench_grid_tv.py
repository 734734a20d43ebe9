#!/usr/bin/env python
"""Developer benchmark of the total-variation regulariser (lightplane_amd/regularizers.py) on one MI355X.

    python scripts/bench_grid_tv.py [--reps 20] [--warmup 3] [--out profiles/grid_tv_bench.txt]

Per workload (the cfg-5 voxel grid 256^3 x 32, a batched triplane B = 8 of 3 x 512^2 x 32, a small 64^3 x 16 grid) and p = 1:
  fused          add_grid_tv_grad_: loss value + gradient accumulated, ONE sweep
  forward        grid_tv_loss alone (no autograd)
  autograd       grid_tv_loss(...).backward(): forward sweep + gather backward (overwrite) + autograd's bookkeeping
  torch          the same loss written in PyTorch on the [B, D, H, W, C] views, forward + backward (where it fits)
  clone          a clone() of the grid tensors: one read + one write of the grid, the bandwidth yardstick
Times are device-event medians over --reps calls after --warmup calls; memory is torch.cuda.max_memory_allocated above what was
allocated before the call.  The script needs a GPU and fails without one.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lightplane_amd as lp  # noqa: E402

WORKLOADS = {
    "cfg5_voxel_256^3x32": [(1, 256, 256, 256, 32)],
    "triplane_B8_3x512^2x32": [(8, 1, 512, 512, 32), (8, 512, 1, 512, 32), (8, 512, 512, 1, 32)],
    "small_64^3x16": [(1, 64, 64, 64, 16)],
}


def torch_tv(grids, p=1):
    total = 0.0
    for g in grids:
        for ax in (1, 2, 3):
            n = g.shape[ax]
            if n > 1:
                d = g.narrow(ax, 1, n - 1) - g.narrow(ax, 0, n - 1)
                total = total + (d.abs() if p == 1 else d * d).mean()
    return total


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--p", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated workload names")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_grid_tv.py measures on a GPU; there is nothing to fall back to"
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                                cwd=os.path.dirname(os.path.abspath(__file__))).stdout.strip() or "n/a"
    except OSError:
        commit = "n/a"
    say(f"# grid_tv bench  {time.strftime('%Y-%m-%d')}  commit {commit}  {torch.cuda.get_device_name(0)}  library src {lp._lib.build_info()['src_hash'][:16]}")
    say(f"# p = {a.p}, median of {a.reps} calls after {a.warmup} warm-up calls (device events); min / max in brackets; mem = peak bytes above the start")
    for name, shapes in WORKLOADS.items():
        if a.only and name not in a.only.split(","):
            continue
        gen = torch.Generator(device=dev).manual_seed(0)
        grids = [torch.randn(*s, device=dev, generator=gen) for s in shapes]
        grads = [torch.zeros_like(g) for g in grids]
        nbytes = sum(g.numel() * 4 for g in grids)
        ws = lp.grid_tv_workspace_bytes([list(s) for s in shapes])
        say(f"\n{name}: {nbytes / 2**20:.1f} MiB of grid, workspace {ws} bytes")
        res = {}

        def clone():
            return [g.clone() for g in grids]

        def fused():
            return lp.add_grid_tv_grad_(grids, grads, weight=1e-3, p=a.p)

        def forward():
            with torch.no_grad():
                return lp.grid_tv_loss(grids, p=a.p)

        leaves = [g.detach().requires_grad_(True) for g in grids]

        def autograd():
            for t in leaves:
                t.grad = None
            lp.grid_tv_loss(leaves, p=a.p).backward()

        def torch_expr():
            for t in leaves:
                t.grad = None
            torch_tv(leaves, a.p).backward()

        for key, fn in (("clone", clone), ("fused", fused), ("forward", forward), ("autograd", autograd), ("torch", torch_expr)):
            try:
                res[key] = timed(fn, a.reps, a.warmup)
            except torch.cuda.OutOfMemoryError:
                res[key] = None
                torch.cuda.empty_cache()
            for t in leaves:
                t.grad = None
        c = res["clone"][0]
        for key in ("clone", "fused", "forward", "autograd", "torch"):
            r = res[key]
            if r is None:
                say(f"  {key:9s} does not fit (out of memory)")
                continue
            # bytes the algorithm needs: clone 2 x grid; fused 3 x (read grid, read + write gradient); forward 1 x; backward 1 + 1
            need = {"clone": 2, "fused": 3, "forward": 1, "autograd": 3, "torch": None}[key]
            rate = f"{need * nbytes / (r[0] * 1e-3) / 1e12:5.2f} TB/s of needed bytes" if need else " " * 27
            say(f"  {key:9s} {r[0]:9.3f} ms [{r[1]:.3f} .. {r[2]:.3f}]  {r[0] / c:6.2f} x clone  {rate}  mem +{r[3] / 2**20:9.1f} MiB")
        # same numbers? (the PyTorch expression and the kernels on the same tensors)
        with torch.no_grad():
            same = abs(float(torch_tv(grids, a.p)) - float(lp.grid_tv_loss(grids, p=a.p))) / max(float(torch_tv(grids, a.p)), 1e-30) \
                if res["torch"] is not None else float("nan")
        say(f"  loss: kernels vs the PyTorch expression (fp32) differ by {same:.1e} relative")
        del grids, grads, leaves
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

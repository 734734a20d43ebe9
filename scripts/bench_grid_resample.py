#!/usr/bin/env python
"""Developer benchmark of the grid-list resampling (lightplane_amd/resample.py) on one MI355X.

    python scripts/bench_grid_resample.py [--reps 20] [--warmup 3] [--out profiles/grid_resample_bench.txt]

Per workload (a 128^3 x 32 voxel grid -> 256^3 x 32; a 256^2 x 32 triplane -> 512^2), factor 2, align_corners off:
  clone          a clone() of the RESULT: one read + one write of the output's bytes, the bandwidth yardstick
  forward        lp.grid_resample without autograd: reads the input (1 / 8 of the output for a voxel grid, 1 / 4 for a plane), writes the
                 output
  adjoint        lp_grid_resample_backward (overwrite) into preallocated gradient buffers: reads the output-sized upstream gradient,
                 writes the input-sized gradient
  torch          the reference's expression: permute -> F.interpolate -> permute -> contiguous (forward only, as grid_up_sample runs)
Times are device-event medians over --reps calls after --warmup calls; memory is torch.cuda.max_memory_allocated above what was
allocated before the call.  The script needs a GPU and fails without one.
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lightplane_amd as lp  # noqa: E402
from lightplane_amd import _lib, grids as lp_grids  # noqa: E402

WORKLOADS = {
    "voxel_128^3x32_to_256^3": [(1, 128, 128, 128, 32)],
    "triplane_3x256^2x32_to_512^2": [(1, 1, 256, 256, 32), (1, 256, 1, 256, 32), (1, 256, 256, 1, 32)],
}


def torch_up_sample(g, factor=2.0, align_corners=False):
    """the reference helper's expression for one [B, D, H, W, C] grid"""
    sing = [i for i, s in enumerate(g.shape[1:-1]) if s == 1]
    if not sing:
        return F.interpolate(g.permute(0, 4, 1, 2, 3), scale_factor=factor, mode="trilinear",
                             align_corners=align_corners).permute(0, 2, 3, 4, 1).contiguous()
    d = sing[0] + 1
    return F.interpolate(g.squeeze(d).permute(0, 3, 1, 2), scale_factor=factor, mode="bilinear",
                         align_corners=align_corners).permute(0, 2, 3, 1).unsqueeze(d).contiguous()


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


def abi_list(tensors):
    C = tensors[0].shape[-1]
    return _lib.make_grid_list([t.view(-1, C) for t in tensors], [lp_grids.GridDesc(*t.shape[:4], 0) for t in tensors], C, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated workload names")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_grid_resample.py measures on a GPU; there is nothing to fall back to"
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# grid_resample bench  {time.strftime('%Y-%m-%d')}  {torch.cuda.get_device_name(0)}  library src {_lib.build_info()['src_hash'][:16]}")
    say(f"# factor 2, align_corners off; median of {a.reps} calls after {a.warmup} warm-up calls (device events); min / max in brackets; "
        "mem = peak bytes above the start")
    for name, shapes in WORKLOADS.items():
        if a.only and name not in a.only.split(","):
            continue
        gen = torch.Generator(device=dev).manual_seed(0)
        grids = [torch.randn(*s, device=dev, generator=gen) for s in shapes]
        with torch.no_grad():
            outs = lp.grid_resample(grids, scale_factor=2.0)
        in_bytes = sum(g.numel() * 4 for g in grids)
        out_bytes = sum(o.numel() * 4 for o in outs)
        say(f"\n{name}: input {in_bytes / 2**20:.1f} MiB -> output {out_bytes / 2**20:.1f} MiB")
        g_in = [torch.empty_like(g) for g in grids]
        src, dst = abi_list(g_in), abi_list(outs)
        co = (ctypes.c_float * (3 * len(grids)))(*([0.5] * (3 * len(grids))))
        stream = _lib.current_stream(dev)

        def clone():
            return [o.clone() for o in outs]

        def forward():
            with torch.no_grad():
                return lp.grid_resample(grids, scale_factor=2.0)

        def adjoint():
            _lib.check(_lib.lib().lp_grid_resample_backward(ctypes.byref(src), ctypes.byref(dst), 0, co, 0, stream), "adjoint")

        def torch_expr():
            with torch.no_grad():
                return [torch_up_sample(g) for g in grids]

        res = {}
        for key, fn in (("clone", clone), ("forward", forward), ("adjoint", adjoint), ("torch", torch_expr)):
            try:
                res[key] = timed(fn, a.reps, a.warmup)
            except torch.cuda.OutOfMemoryError:
                res[key] = None
                torch.cuda.empty_cache()
        c = res["clone"][0]
        need = {"clone": 2 * out_bytes, "forward": in_bytes + out_bytes, "adjoint": in_bytes + out_bytes, "torch": in_bytes + out_bytes}
        for key in ("clone", "forward", "adjoint", "torch"):
            r = res[key]
            if r is None:
                say(f"  {key:8s} does not fit (out of memory)")
                continue
            say(f"  {key:8s} {r[0]:9.3f} ms [{r[1]:.3f} .. {r[2]:.3f}]  {r[0] / c:6.2f} x clone  {need[key] / (r[0] * 1e-3) / 1e12:5.2f} TB/s of needed bytes"
                f"  mem +{r[3] / 2**20:9.1f} MiB")
        with torch.no_grad():
            worst = max(float((o - torch_up_sample(g)).abs().max() / o.abs().max()) for o, g in zip(outs, grids))
        say(f"  forward: kernels vs the PyTorch expression (fp32) differ by {worst:.1e} of the largest value")
        del grids, outs, g_in
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

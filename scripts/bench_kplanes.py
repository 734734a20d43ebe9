#!/usr/bin/env python
"""Developer benchmark of the space-time plane encoding (lightplane_amd/kplanes.py) on one MI355X.

    python scripts/bench_kplanes.py [--reps 7] [--warmup 3] [--out profiles/kplanes_bench.txt]

S = 4 scales of 64, 128, 256 and 512 vertices per axis, C = 16 and 32 channels, static (3 planes per scale) and dynamic (6 planes,
150 vertices on t, one timestamp per ray), at 2^18 and 2^20 points -- [R, 128, 3] samples along random rays through the box, sorted by
depth -- and at 2^20 randomly permuted points, in ONE process, the paths alternating on the same inputs:
  torch   the composition a user would write: per plane ``permute`` to [1, C, n_v, n_u] + ``F.grid_sample(align_corners=True,
          padding_mode="border")``, a product over the planes, ``cat`` over the scales, and its autograd
  fused   lp.kplanes_encode
for the forward alone (no_grad) and for forward + backward with the gradient to the planes (the training loop; the points get none).
Device-event medians over --reps calls after --warmup calls, two passes per path (their spread is the run-to-run spread); memory is
torch.cuda.max_memory_allocated above what was allocated before the calls (results and gradients included), beside the bound the
fused path has to meet: the forward allocates ``out`` (4 S C bytes per point) and nothing else, forward + backward adds the gradient
of the planes only (the upstream gradient is the benchmark's input, and the points ask for no gradient).  The bound allows 1 MiB per
tensor for the caching allocator, which hands out a whole block where splitting it would leave less than that.
Permuted points have no runs of consecutive points in one cell, so the last rows show what the run merge of the plane gradient (and the
locality of the order) buys.  It needs a GPU and fails without one.
"""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lightplane_amd as lp  # noqa: E402
from lightplane_amd import _lib  # noqa: E402

N_PTS, SPATIAL, TEMPORAL = 128, (64, 128, 256, 512), 150
ALLOC_SLACK = 1 << 20   # the caching allocator does not split a block when the remainder is under 1 MiB
AXES = ((0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (2, 3))


def timed(fn, reps, warmup, release):
    """(median ms, min ms, max ms, peak bytes above the starting allocation) of fn(); release() drops what a call leaves behind"""
    for _ in range(warmup):
        fn()
    release()
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


def torch_encode(points, times, planes, lay):
    """the encoding as a user would compose it (one scene, no mask, no contraction)"""
    R, N = points.shape[:2]
    coords = points if times is None else torch.cat([points, times[:, None, None].expand(R, N, 1)], dim=-1)
    out = []
    for s in range(lay.n_scales):
        res = [lay.spatial[s]] * 3 + ([lay.temporal[s]] if lay.temporal else [])
        prod = None
        for j, (u, v) in enumerate(AXES[:lay.n_planes]):
            first = lay.offsets[s][j]
            image = planes[0, first:first + res[u] * res[v]].reshape(1, res[v], res[u], lay.channels).permute(0, 3, 1, 2)
            val = F.grid_sample(image, coords[..., [u, v]][None], mode="bilinear", padding_mode="border", align_corners=True)
            val = val[0].permute(1, 2, 0)
            prod = val if prod is None else prod * val
        out.append(prod)
    return torch.cat(out, dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kplanes.py measures on a GPU; there is nothing to fall back to"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# kplanes bench  {time.strftime('%Y-%m-%d')}  {torch.cuda.get_device_name(0)}  library src {_lib.build_info()['src_hash'][:16]}")
    say(f"# lp.kplanes_encode against the same encoding composed from permute + grid_sample + product + cat (and its autograd); median of "
        f"{a.reps} calls after {a.warmup} warm-up calls (device events), the paths alternating, two passes each; min / max in brackets; "
        "mem = peak bytes above the start, bound = what the fused path may allocate")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    misses = []
    for channels in (16, 32):
        for dynamic in (False, True):
            lay = lp.kplanes_layout(SPATIAL, TEMPORAL if dynamic else None, channels)
            planes = lp.init_kplanes(lay, 1, device=dev, generator=gen)
            if dynamic:   # (space-time planes of exactly 1 would make their gradient the static field's: draw them too)
                planes = torch.rand(planes.shape, device=dev, generator=gen) * 0.4 + 0.8
            planes.requires_grad_(True)
            for n_points, permuted in ((1 << 18, False), (1 << 20, False), (1 << 20, True)):
                R = n_points // N_PTS
                start, end = (torch.rand(R, 1, 3, device=dev, generator=gen) * 1.8 - 0.9 for _ in range(2))
                t = torch.rand(R, N_PTS, 1, device=dev, generator=gen).sort(dim=1).values
                pts = start + t * (end - start)
                if permuted:
                    pts = pts.reshape(-1, 3)[torch.randperm(n_points, device=dev, generator=gen)].reshape(pts.shape).contiguous()
                times = torch.rand(R, device=dev, generator=gen) * 2 - 1 if dynamic else None
                gidx = torch.zeros(R, dtype=torch.int32, device=dev)   # (int32 is what the kernels read: no converted copy)
                up = torch.randn(R, N_PTS, lay.out_channels, device=dev, generator=gen)
                fused = lambda p, pl: lp.kplanes_encode(p, times, pl, gidx, lay)  # noqa: E731
                paths = {"torch": lambda p, pl: torch_encode(p, times, pl, lay), "fused": fused}
                out_bytes, plane_bytes = n_points * lay.out_channels * 4, planes.numel() * 4

                def forward(fn):
                    with torch.no_grad():
                        return fn(pts, planes.detach())

                def fwd_bwd(fn):
                    planes.grad = None
                    fn(pts, planes).backward(up)   # (the upstream gradient is an input: nothing but the op's own tensors is allocated)
                    return planes.grad

                say(f"\nC = {channels}, {'dynamic' if dynamic else 'static'} ({lay.n_planes} planes x {lay.n_scales} scales, "
                    f"{plane_bytes / 2 ** 20:.1f} MiB of planes), {n_points} points = {R} rays x {N_PTS}" + (", PERMUTED" if permuted else ""))
                for what, run, bound in (("forward", forward, out_bytes + ALLOC_SLACK), ("forward + backward", fwd_bwd, out_bytes + plane_bytes + 2 * ALLOC_SLACK)):
                    res = {k: [] for k in paths}
                    for key, fn in tuple(paths.items()) * 2:
                        res[key].append(timed(lambda: run(fn), a.reps, a.warmup, lambda: setattr(planes, "grad", None)))
                        planes.grad = None
                    for key in paths:
                        for i, r in enumerate(res[key]):
                            say(f"  {what:18s} {key:6s} pass {i}: {r[0]:9.3f} ms [{r[1]:.3f} .. {r[2]:.3f}]  mem +{r[3] / 2 ** 20:9.1f} MiB")
                    med = {k: statistics.median(r[0] for r in res[k]) for k in paths}
                    mem = {k: max(r[3] for r in res[k]) for k in paths}
                    spread = max(abs(res[k][0][0] - res[k][1][0]) / med[k] for k in paths)
                    say(f"  {what:18s} torch / fused: time {med['torch'] / med['fused']:.2f} x ({med['torch']:.3f} -> {med['fused']:.3f} ms; passes "
                        f"differ by up to {100 * spread:.1f} %), peak memory {mem['torch'] / max(mem['fused'], 1):.2f} x "
                        f"({mem['torch'] / 2 ** 20:.1f} -> {mem['fused'] / 2 ** 20:.1f} MiB; bound {bound / 2 ** 20:.1f} MiB: "
                        f"{'met' if mem['fused'] <= bound else 'MISSED'})")
                    if med["fused"] > med["torch"] * (1 + spread):
                        misses.append(f"C = {channels}, {'dynamic' if dynamic else 'static'}, {n_points} points{' permuted' if permuted else ''}, "
                                      f"{what} ({med['torch']:.3f} -> {med['fused']:.3f} ms)")
                    got, ref = run(paths["torch"]).detach().clone(), run(fused).detach()
                    say(f"  {what:18s} torch differs from fused by at most {float((got - ref).abs().max()) / float(ref.abs().max()):.2e} of the "
                        "tensor's max |value| (both fp32)")
    say("\n# fused slower than the PyTorch composition beyond the spread: " + ("nowhere" if not misses else "; ".join(misses)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

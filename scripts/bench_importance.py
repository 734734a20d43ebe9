#!/usr/bin/env python
"""Developer benchmark of importance resampling (lightplane_amd/importance.py) on one MI355X.

    python scripts/bench_importance.py [--reps 5] [--warmup 2] [--out profiles/importance_bench.txt]

At 65 536 rays, S = 128 coarse samples and N = 128 new ones per ray, in ONE process, the two paths alternating:
  torch   the same computation composed from PyTorch ops -- ``cumsum`` of the padded weights, ``searchsorted`` of the targets, two
          ``gather`` pairs, the interpolation, ``cat`` + ``sort`` for the merge, the differences, the point formula -- and its autograd
  fused   lp.importance_samples
for the forward alone (no_grad) and for forward + backward with gradients to the ray origins and directions.  Protocol of
scripts/bench_compositing.py: device-event medians over --reps calls after --warmup calls, two passes per path; memory is
torch.cuda.max_memory_allocated above what was allocated before the calls (results and gradients included; the report says how much of
the peak they are).  The fused rows also give the fraction of the achievable HBM rate (6.29 TB/s: the measured float4 copy rate of the
chip) that the algorithmic bytes imply: depths, weights and jitter read once, the three results written once; in the backward the
upstream gradient of the points and the result depths read once.
It needs a GPU and fails without one.
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lightplane_amd as lp  # noqa: E402
from lightplane_amd import _lib  # noqa: E402

R, S, N = 65536, 128, 128
HBM_BYTES_PER_S = 6.29e12
PAD = 1e-5


def timed(fn, reps, warmup, clear=None):
    """(median ms, min ms, max ms, peak bytes above the starting allocation) of fn()"""
    for _ in range(warmup):
        fn()
    if clear is not None:
        clear()
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


def torch_importance(origins, directions, depths, weights, jitter):
    """the definition in PyTorch ops, as a user would write it (sample positions detached)"""
    with torch.no_grad():
        e = torch.cat([depths[:, :1], 0.5 * (depths[:, :-1] + depths[:, 1:]), depths[:, -1:]], dim=1)
        p = torch.where(weights > 0, weights, torch.zeros_like(weights)) + PAD
        C = torch.nn.functional.pad(torch.cumsum(p, dim=1), (1, 0))
        k = torch.arange(N, device=depths.device, dtype=torch.float32)
        x = ((k[None] + jitter) / N) * C[:, -1:]
        j = (torch.searchsorted(C, x, right=True) - 1).clamp(0, S - 1)
        c0, c1 = C.gather(1, j), C.gather(1, j + 1)
        a = ((x - c0) / (c1 - c0)).nan_to_num(0.0).clamp(0, 1)
        e0, e1 = e.gather(1, j), e.gather(1, j + 1)
        t = torch.minimum(torch.maximum(e0 + a * (e1 - e0), e0), e1)
        out = torch.sort(torch.cat([depths, t], dim=1), dim=1).values
        diff = out[:, 1:] - out[:, :-1]
        deltas = torch.cat([diff[:, :1], diff], dim=1)
    points = out[..., None] * directions[:, None] + origins[:, None]
    return points, out, deltas


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_importance.py measures on a GPU; there is nothing to fall back to"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# importance bench  {time.strftime('%Y-%m-%d')}  {torch.cuda.get_device_name(0)}  library src {_lib.build_info()['src_hash'][:16]}")
    say(f"# lp.importance_samples against the same computation composed from PyTorch ops (and its autograd); median of {a.reps} calls "
        f"after {a.warmup} warm-up calls (device events), the two paths alternating, two passes each; min / max in brackets; mem = peak "
        "bytes above the start")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    deltas = torch.rand(R, S, device=dev, generator=gen) * 0.05 + 0.01
    depths = 0.5 + torch.cumsum(deltas, -1)
    # the weights of a ray that meets a surface: a bump of width ~ 4 samples somewhere along it, on a floor of 1e-4
    centre = torch.rand(R, 1, device=dev, generator=gen) * S
    weights = 0.25 * torch.exp(-0.5 * ((torch.arange(S, device=dev)[None] - centre) / 2.0) ** 2) + 1e-4
    jitter = torch.rand(R, N, device=dev, generator=gen)
    origins = torch.randn(R, 3, device=dev, generator=gen)
    directions = torch.nn.functional.normalize(torch.randn(R, 3, device=dev, generator=gen), dim=-1)
    up = torch.randn(R, S + N, 3, device=dev, generator=gen)
    leaves = [origins.clone().requires_grad_(True), directions.clone().requires_grad_(True)]
    rays_plain = lp.Rays(directions=directions, origins=origins, grid_idx=torch.zeros(R, dtype=torch.int32, device=dev),
                         near=torch.zeros(R, device=dev), far=torch.ones(R, device=dev))
    rays_grad = lp.Rays(directions=leaves[1], origins=leaves[0], grid_idx=rays_plain.grid_idx, near=rays_plain.near, far=rays_plain.far)

    def fused(o, d):
        rays = rays_plain if o is origins else rays_grad
        return tuple(lp.importance_samples(rays, depths, weights, N, pad=PAD, jitter=jitter))

    def torch_path(o, d):
        return torch_importance(o, d, depths, weights, jitter)

    def forward(fn):
        with torch.no_grad():
            return fn(origins, directions)

    def clear():
        for t in leaves:
            t.grad = None

    def fwd_bwd(fn):
        clear()
        out = fn(*leaves)
        (out[0] * up).sum().backward()
        return [t.grad for t in leaves]

    say(f"\nimportance_samples, {R} rays, S = {S} coarse + N = {N} new samples per ray")
    out_bytes = 4 * R * (S + N) * 5
    fwd_bytes = 4 * R * (2 * S + N + 6) + out_bytes
    bwd_bytes = 4 * R * ((S + N) * 4 + 6)
    misses = []
    for what, run, nbytes, kept in (("forward", forward, fwd_bytes, out_bytes), ("forward + backward", fwd_bwd, fwd_bytes + bwd_bytes, out_bytes)):
        res = {"torch": [], "fused": []}
        for key, fn in (("torch", torch_path), ("fused", fused)) * 2:
            res[key].append(timed(lambda: run(fn), a.reps, a.warmup, clear))
        for key in ("torch", "fused"):
            for i, r in enumerate(res[key]):
                say(f"  {what:22s} {key:8s} pass {i}: {r[0]:9.3f} ms [{r[1]:.3f} .. {r[2]:.3f}]  mem +{r[3] / 2 ** 20:9.1f} MiB")
        tt, tf = (statistics.median(r[0] for r in res[k]) for k in ("torch", "fused"))
        mt, mf = (max(r[3] for r in res[k]) for k in ("torch", "fused"))
        say(f"  {what:22s} torch / fused: time {tt / tf:.2f} x ({tt:.3f} -> {tf:.3f} ms), peak memory {mt / max(mf, 1):.2f} x "
            f"({mt / 2 ** 20:.1f} -> {mf / 2 ** 20:.1f} MiB); {nbytes / 2 ** 20:.0f} MiB of algorithmic traffic = "
            f"{nbytes / (tf * 1e-3) / HBM_BYTES_PER_S:.2f} of the achievable HBM rate")
        say(f"  {what:22s} of which results handed back: {kept / 2 ** 20:.1f} MiB on either path; beyond them "
            f"{(mt - kept) / 2 ** 20:.1f} -> {(mf - kept) / 2 ** 20:.1f} MiB")
        x, y = run(torch_path), run(fused)
        names = ("points", "depths", "deltas") if what == "forward" else ("d origins", "d directions")
        diffs = ", ".join(f"{n} {float((p - q).abs().max()) / max(float(p.abs().max()), 1e-30):.2e}" for n, p, q in zip(names, x, y))
        say(f"  {what:22s} the two paths differ by at most (of a tensor's max |value|; both are fp32, and where a bin is nearly empty "
            f"the inverse CDF is steep): {diffs}")
        if tf > tt:
            misses.append(f"{what}: not faster ({tt:.3f} -> {tf:.3f} ms)")
    say("\n# fused slower than the PyTorch composition: " + ("nowhere" if not misses else "; ".join(misses)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

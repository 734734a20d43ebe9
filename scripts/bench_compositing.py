#!/usr/bin/env python
"""Developer benchmark of the modular march (lightplane_amd/compositing.py) on one MI355X.

    python scripts/bench_compositing.py [--reps 5] [--warmup 2] [--out profiles/compositing_bench.txt]

At 65 536 rays x 128 samples, C = 3 and 32 feature channels, in ONE process, the two paths alternating:
  torch   the same computation composed from PyTorch ops -- ``cumsum(pad(opacity * delta))``, ``exp``, the difference of neighbours,
          three weighted sums -- and its autograd
  fused   lp.composite_samples
for the forward alone (no_grad) and for forward + backward with gradients to all four inputs.  Times are device-event medians over
--reps calls after --warmup calls, two passes per path; memory is torch.cuda.max_memory_allocated above what was allocated before the
calls with no result or gradient of an earlier call alive (results and gradients included; the report also says how much of the peak
they are, since either path has to allocate them).  The fused rows also give the fraction of the achievable HBM rate (6.29 TB/s: the measured
float4 copy rate of the chip) that the algorithmic bytes imply: every input once in the forward; opacity and deltas twice, everything
else once, and every gradient written once in the backward.

For context, the chain ``lp.ray_samples -> lp.lightplane_eval_mlp -> lp.composite_samples`` next to ``lp.lightplane_renderer`` on the
same rays (a 128^2 x 16 triplane, the 2/2/2 x 32 decoder, 3 colours): forward, and forward + backward into grids and decoder.
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

R, S = 65536, 128
HBM_BYTES_PER_S = 6.29e12


def timed(fn, reps, warmup, clear=None):
    """(median ms, min ms, max ms, peak bytes above the starting allocation) of fn().  ``clear()`` drops what a call leaves behind (the
    gradients on the leaves) before the starting allocation is read: the peak then counts everything a call allocates, its results and
    gradients included."""
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


def torch_composite(opacity, features, depths, deltas):
    od = opacity * deltas
    nlt = torch.cumsum(torch.nn.functional.pad(od, (1, 0)), dim=-1)
    t = torch.exp(-nlt)
    w = t[:, :-1] - t[:, 1:]
    return (depths * w).sum(-1), nlt[:, -1], (features * w[..., None]).sum(-2)


def compare(say, what, fns, reps, warmup, bytes_moved=None, clear=None, kept=0):
    """fns: {"torch" | "renderer": fn, "fused" | "chain": fn}; returns (reference ms, new ms, reference peak, new peak).  ``kept``: the
    bytes of results and gradients a call hands back, which either path has to allocate; the peak beyond them is a path's own."""
    (ka, fa), (kb, fb) = fns.items()
    res = {ka: [], kb: []}
    for key, fn in ((ka, fa), (kb, fb), (ka, fa), (kb, fb)):
        res[key].append(timed(fn, reps, warmup, clear))
    for key in (ka, kb):
        for i, r in enumerate(res[key]):
            say(f"  {what:22s} {key:8s} pass {i}: {r[0]:9.3f} ms [{r[1]:.3f} .. {r[2]:.3f}]  mem +{r[3] / 2 ** 20:9.1f} MiB")
    ta, tb = (statistics.median(r[0] for r in res[k]) for k in (ka, kb))
    ma, mb = (max(r[3] for r in res[k]) for k in (ka, kb))
    hbm = ""
    if bytes_moved is not None:
        hbm = f"; {bytes_moved / 2 ** 20:.0f} MiB of algorithmic traffic = {bytes_moved / (tb * 1e-3) / HBM_BYTES_PER_S:.2f} of the achievable HBM rate"
    say(f"  {what:22s} {ka} / {kb}: time {ta / tb:.2f} x ({ta:.3f} -> {tb:.3f} ms), peak memory {ma / max(mb, 1):.2f} x "
        f"({ma / 2 ** 20:.1f} -> {mb / 2 ** 20:.1f} MiB){hbm}")
    if kept:
        say(f"  {what:22s} of which results and gradients handed back: {kept / 2 ** 20:.1f} MiB on either path; beyond them "
            f"{(ma - kept) / 2 ** 20:.1f} -> {(mb - kept) / 2 ** 20:.1f} MiB")
    return ta, tb, ma, mb


def bench_composite(say, C, reps, warmup):
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(C)
    deltas = torch.rand(R, S, device=dev, generator=gen) * 0.05 + 0.01
    depths = 0.5 + torch.cumsum(deltas, -1)
    opacity = torch.rand(R, S, device=dev, generator=gen) * 2.0
    features = torch.randn(R, S, C, device=dev, generator=gen)
    ups = (torch.randn(R, device=dev, generator=gen), torch.randn(R, device=dev, generator=gen), torch.randn(R, C, device=dev, generator=gen))
    leaves = [t.clone().requires_grad_(True) for t in (opacity, features, depths, deltas)]

    def forward(fn):
        with torch.no_grad():
            return fn(opacity, features, depths, deltas)

    def fwd_bwd(fn):
        for t in leaves:
            t.grad = None
        out = fn(*leaves)
        sum((o * u).sum() for o, u in zip(out, ups)).backward()
        return [t.grad for t in leaves]

    say(f"\ncomposite_samples, {R} rays x {S} samples, C = {C}")
    fwd_bytes = 4 * (R * S * (3 + C) + R * (2 + C))
    bwd_bytes = 4 * (R * S * (2 * 2 + 1 + C) + R * (2 + C) + R * S * (3 + C))
    def clear():
        for t in leaves:
            t.grad = None

    out_bytes, grad_bytes = 4 * R * (2 + C), 4 * R * S * (3 + C)
    rows = {}
    for what, run, nbytes, kept in (("forward", forward, fwd_bytes, out_bytes), ("forward + backward", fwd_bwd, fwd_bytes + bwd_bytes, grad_bytes)):
        rows[what] = compare(say, what, {"torch": lambda: run(torch_composite), "fused": lambda: run(lp.composite_samples)}, reps, warmup,
                             nbytes, clear, kept)
        a, b = run(torch_composite), run(lp.composite_samples)
        worst = max(float((x - y).abs().max()) / max(float(x.abs().max()), 1e-30) for x, y in zip(a, b))
        say(f"  {what:22s} the two paths differ by at most {worst:.2e} of a result's max |value|")
    return rows


def bench_chain(say, reps, warmup):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(0)
    chn, res = 16, 128
    shapes = [(1, 1, res, res, chn), (1, res, 1, res, chn), (1, res, res, 1, chn)]
    grids = [(0.1 * torch.randn(*s, generator=gen)).to(dev).requires_grad_(True) for s in shapes]
    mod = lp.LightplaneRenderer(num_samples=S, color_chn=3, grid_chn=chn, mlp_hidden_chn=32, opacity_init_bias=-2.0, gain=1.0,
                                ray_embedding_num_harmonics=None).to(dev)
    dec = mod.get_decoder_params()
    o = torch.randn(R, 3, generator=gen)
    o = 2.5 * o / o.norm(dim=-1, keepdim=True)
    d = -o / o.norm(dim=-1, keepdim=True) + 0.2 * torch.randn(R, 3, generator=gen)
    rays = lp.Rays(directions=d.to(dev), origins=o.to(dev), grid_idx=torch.zeros(R, dtype=torch.int32, device=dev),
                   near=torch.full((R,), 1.2, device=dev), far=torch.full((R,), 3.8, device=dev),
                   encoding=torch.randn(R, mod.rays_encoding_dim, generator=gen).to(dev))
    ups = (torch.randn(R, generator=gen).to(dev), torch.randn(R, generator=gen).to(dev), torch.randn(R, 3, generator=gen).to(dev))

    def renderer():
        return lp.lightplane_renderer(rays, grids, dec, num_samples=S, gain=1.0)

    def chain():
        s = lp.ray_samples(rays, S)
        opacity, color = lp.lightplane_eval_mlp(s.points, grids, rays.grid_idx, dec, rays.encoding, 1.0)
        return lp.composite_samples(opacity, color, s.depths, s.deltas)

    def forward(fn):
        with torch.no_grad():
            return fn()

    def fwd_bwd(fn):
        for t in grids + [mod.mlp_params]:
            t.grad = None
        sum((o * u).sum() for o, u in zip(fn(), ups)).backward()
        return [t.grad for t in grids + [mod.mlp_params]]

    say(f"\nfor context: ray_samples -> lightplane_eval_mlp -> composite_samples next to lightplane_renderer, {R} rays x {S} samples, "
        f"{res}^2 x {chn} triplane, 2/2/2 x 32 decoder")
    def clear():
        for t in grids + [mod.mlp_params]:
            t.grad = None

    for what, run in (("forward", forward), ("forward + backward", fwd_bwd)):
        compare(say, what, {"renderer": lambda: run(renderer), "chain": lambda: run(chain)}, reps, warmup, clear=clear)
        a, b = run(renderer), run(chain)
        worst = max(float((x - y).abs().max()) / max(float(x.abs().max()), 1e-30) for x, y in zip(a, b))
        say(f"  {what:22s} the two paths differ by at most {worst:.2e} of a result's max |value|")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_compositing.py measures on a GPU; there is nothing to fall back to"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# compositing bench  {time.strftime('%Y-%m-%d')}  {torch.cuda.get_device_name(0)}  library src {_lib.build_info()['src_hash'][:16]}")
    say(f"# lp.composite_samples against the same computation composed from PyTorch ops (and its autograd); median of {a.reps} calls "
        f"after {a.warmup} warm-up calls (device events), the two paths alternating, two passes each; min / max in brackets; mem = peak "
        "bytes above the start")
    misses = []
    for C in (3, 32):
        for what, (tt, tf, mt, mf) in bench_composite(say, C, a.reps, a.warmup).items():
            if tf > tt:
                misses.append(f"C = {C} {what}: not faster ({tt:.3f} -> {tf:.3f} ms)")
            if mt < 3 * mf:
                misses.append(f"C = {C} {what}: peak memory only {mt / max(mf, 1):.2f} x lower")
    bench_chain(say, a.reps, a.warmup)
    say("\n# expectations missed (fused not faster; peak memory not three times lower): " + ("none" if not misses else "; ".join(misses)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

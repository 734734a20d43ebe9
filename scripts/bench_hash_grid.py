#!/usr/bin/env python
"""Developer benchmark of the hash-grid encoding (lightplane_amd/hash_grid.py) on one MI355X.

    python scripts/bench_hash_grid.py [--reps 7] [--warmup 3] [--out profiles/hash_grid_bench.txt]

At 2^18 and 2^20 points -- [R, 128, 3] samples along random rays through the box, sorted by depth -- with L = 16 levels of F = 2
features from 16 to 2048, for a 2^19-entry table (the Instant-NGP default: 48 MB, larger than an L2) and a 2^14-entry one (1.6 MB: it
lives in L2), in ONE process, the paths alternating:
  torch   the same encoding from PyTorch ops and its autograd: index arithmetic, eight ``table[idx]`` gathers per level, a weighted
          sum, ``cat`` (the backward is autograd's ``index_put_(accumulate=True)``)
  fused   lp.hash_grid_encode
for the forward alone (no_grad) and for forward + backward with the gradient to the table (the training loop; the points get none).
Device-event medians over --reps calls after --warmup calls, two passes per path (their spread is the run-to-run spread); memory is
torch.cuda.max_memory_allocated above what was allocated before the calls (results and gradients included).  The fused rows also give
the fraction of the achievable HBM rate (6.29 TB/s: the measured float4 copy rate of the chip) that the bytes the algorithm asks for
imply -- points and upstream rows read once per level, results written once, 8 corner rows of 4 F bytes read (forward) or added
(backward) per point and level; corner rows that hit in a cache are counted all the same, so the figure can exceed what HBM moved.
Last, the table backward alone on the ray-ordered points against the SAME kernel on the same points randomly permuted: permuted
points have no runs of lanes in one cell, so the difference is what the run merge (and the locality of the order) buys.
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

N_PTS, HBM_BYTES_PER_S = 128, 6.29e12


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


def torch_encode(points, table, lay):
    """the encoding as a user would compose it (one scene, no mask, no contraction)"""
    u = ((points + 1) / 2).clamp(0, 1)
    T, out = 1 << lay.log2_table_size, []
    tab = table[0]
    for n_l, off, hashed in zip(lay.resolutions, lay.offsets, lay.hashed):
        x = u * n_l
        i = x.detach().floor().clamp(max=n_l - 1)
        f = x - i
        i = i.long()
        acc = 0
        for k in range(8):
            cx, cy, cz = i[..., 0] + (k & 1), i[..., 1] + ((k >> 1) & 1), i[..., 2] + ((k >> 2) & 1)
            w = (f[..., 0] if k & 1 else 1 - f[..., 0]) * (f[..., 1] if k & 2 else 1 - f[..., 1]) * (f[..., 2] if k & 4 else 1 - f[..., 2])
            if hashed:
                idx = (cx ^ ((cy * 2654435761) & 0xFFFFFFFF) ^ ((cz * 805459861) & 0xFFFFFFFF)) & (T - 1)
            else:
                idx = cx + (n_l + 1) * (cy + (n_l + 1) * cz)
            acc = acc + w[..., None] * tab[off + idx]
        out.append(acc)
    return torch.cat(out, dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_hash_grid.py measures on a GPU; there is nothing to fall back to"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# hash grid bench  {time.strftime('%Y-%m-%d')}  {torch.cuda.get_device_name(0)}  library src {_lib.build_info()['src_hash'][:16]}")
    say(f"# lp.hash_grid_encode against the same encoding composed from PyTorch ops (and its autograd); median of {a.reps} calls after "
        f"{a.warmup} warm-up calls (device events), the paths alternating, two passes each; min / max in brackets; mem = peak bytes above "
        "the start")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    misses = []
    for log2_t in (19, 14):
        lay = lp.hash_grid_layout(16, 2, log2_t, 16, 2048)
        L, F = lay.n_levels, lay.features_per_level
        table = lp.init_hash_grid(lay, 1, scale=1.0, device=dev, generator=gen).requires_grad_(True)
        fused = lambda p, t: lp.hash_grid_encode(p, t, gidx, lay)  # noqa: E731
        paths = {"torch": lambda p, t: torch_encode(p, t, lay), "fused": fused}
        for n_points in (1 << 18, 1 << 20):
            R = n_points // N_PTS
            start, end = (torch.rand(R, 1, 3, device=dev, generator=gen) * 1.8 - 0.9 for _ in range(2))
            t = torch.rand(R, N_PTS, 1, device=dev, generator=gen).sort(dim=1).values
            pts = start + t * (end - start)
            gidx = torch.zeros(R, dtype=torch.int64, device=dev)
            up = torch.randn(R, N_PTS, L * F, device=dev, generator=gen)
            per_level = n_points * L * (12 + 4 * F + 8 * 4 * F)   # point, row of the level, 8 corner rows

            def forward(fn):
                with torch.no_grad():
                    return fn(pts, table.detach())

            def fwd_bwd(fn):
                table.grad = None
                (fn(pts, table) * up).sum().backward()
                return table.grad

            say(f"\nT = 2^{log2_t} ({lay.entries * F * 4 / 2 ** 20:.1f} MiB table, {sum(lay.hashed)} of {L} levels hashed), {n_points} points "
                f"= {R} rays x {N_PTS}")
            for what, run, nbytes in (("forward", forward, per_level), ("forward + backward", fwd_bwd, 2 * per_level)):
                res = {k: [] for k in paths}
                for key, fn in tuple(paths.items()) * 2:
                    res[key].append(timed(lambda: run(fn), a.reps, a.warmup))
                    table.grad = None
                for key in paths:
                    for i, r in enumerate(res[key]):
                        say(f"  {what:18s} {key:6s} pass {i}: {r[0]:9.3f} ms [{r[1]:.3f} .. {r[2]:.3f}]  mem +{r[3] / 2 ** 20:9.1f} MiB")
                med = {k: statistics.median(r[0] for r in res[k]) for k in paths}
                mem = {k: max(r[3] for r in res[k]) for k in paths}
                spread = max(abs(res[k][0][0] - res[k][1][0]) / med[k] for k in paths)
                say(f"  {what:18s} torch / fused: time {med['torch'] / med['fused']:.2f} x ({med['torch']:.3f} -> {med['fused']:.3f} ms; passes "
                    f"differ by up to {100 * spread:.1f} %), peak memory {mem['torch'] / max(mem['fused'], 1):.2f} x "
                    f"({mem['torch'] / 2 ** 20:.1f} -> {mem['fused'] / 2 ** 20:.1f} MiB)")
                if med["fused"] > med["torch"] * (1 + spread):
                    misses.append(f"T = 2^{log2_t}, {n_points} points, {what} ({med['torch']:.3f} -> {med['fused']:.3f} ms)")
                say(f"  {what:18s} fused: {nbytes / 2 ** 20:.0f} MiB asked for = {nbytes / (med['fused'] * 1e-3) / HBM_BYTES_PER_S:.2f} of the "
                    "achievable HBM rate")
                got, ref = run(paths["torch"]).detach().clone(), run(fused).detach()
                say(f"  {what:18s} torch differs from fused by at most {float((got - ref).abs().max()) / float(ref.abs().max()):.2e} of the "
                    "tensor's max |value| (both fp32)")

            # the table backward alone: ray order against a random permutation of the same points (the same kernel)
            perm = torch.randperm(n_points, device=dev, generator=gen)
            res = {"ray order": [], "permuted": []}
            for key, p in (("ray order", pts), ("permuted", pts.reshape(-1, 3)[perm].reshape(pts.shape).contiguous())) * 2:
                out = fused(p, table)
                res[key].append(timed(lambda: torch.autograd.grad(out, table, up, retain_graph=True), a.reps, a.warmup))
                del out
            for key, rs in res.items():
                for i, r in enumerate(rs):
                    say(f"  table backward     {key:9s} pass {i}: {r[0]:9.3f} ms [{r[1]:.3f} .. {r[2]:.3f}]")
            med = {k: statistics.median(r[0] for r in rs) for k, rs in res.items()}
            say(f"  table backward     permuted / ray order: {med['permuted'] / med['ray order']:.2f} x ({med['permuted']:.3f} -> "
                f"{med['ray order']:.3f} ms, zeroing the gradient included)")
    say("\n# fused slower than the PyTorch composition beyond the spread: " + ("nowhere" if not misses else "; ".join(misses)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

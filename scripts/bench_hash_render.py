#!/usr/bin/env python
"""Developer benchmark of the hash-grid render along rays (lightplane_amd/hash_grid.py ``hash_grid_render_samples``) on one MI355X.

    python scripts/bench_hash_render.py [--reps 7] [--warmup 3] [--out profiles/hash_render_bench.txt]

65 536 and 4 096 rays through a hash grid of L = 16 levels of F = 2 features from 16 to 2048, for a 2^14-entry and a 2^19-entry table
and the decoders 2/2/2 x 32 and 1/1/2 x 64, at S = 128 uniform samples (``lp.ray_samples``) and at S = 256 resampled ones
(``lp.importance_samples`` of 192 new samples on 64 coarse ones from the fused op's own coarse weights), in ONE process, the paths
alternating:
  chain   lp.hash_grid_eval_mlp(samples.points) -> lp.composite_samples: opacity [R, S] and colour [R, S, 3] and their gradients are tensors
  fused   lp.hash_grid_render_samples: one launch forward, one backward
for the forward alone (no_grad) and for forward + backward with gradients to the table and the decoder's parameters.  Protocol and
memory accounting: scripts/bench_hash_points.py (device-event medians, two passes per path, peak above the inputs).  The fused peak is
held against what can be said in advance: the three results + chunk_nlt in the forward, + upstream gradients + gradient buffers in
forward + backward -- no [R, S] tensor.  It needs a GPU and fails without one.
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
from scripts.bench_hash_points import make_decoder, timed  # noqa: E402

GAIN = 1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_hash_render.py measures on a GPU; there is nothing to fall back to"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# hash render bench  {time.strftime('%Y-%m-%d')}  {torch.cuda.get_device_name(0)}  library src {_lib.build_info()['src_hash'][:16]}")
    say(f"# lp.hash_grid_render_samples against lp.hash_grid_eval_mlp -> lp.composite_samples on the same samples; median of {a.reps} calls "
        f"after {a.warmup} warm-up calls (device events), the paths alternating, two passes each; min / max in brackets; mem = peak bytes "
        "above the inputs")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    misses, mib = [], 2.0 ** 20
    for log2_t in (14, 19):
        lay = lp.hash_grid_layout(16, 2, log2_t, 16, 2048)
        table = lp.init_hash_grid(lay, 1, scale=1.0, device=dev, generator=gen).requires_grad_(True)
        for shape in ((2, 2, 2, 32), (1, 1, 2, 64)):
            dec = make_decoder(*shape[:3], lay.channels, shape[3], gen, dev)
            params = dec.mlp_params.requires_grad_(True)
            dec = lp.DecoderParams(params, dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
            for R in (65536, 4096):
                start, end = (torch.rand(R, 3, device=dev, generator=gen) * 1.8 - 0.9 for _ in range(2))
                rays = lp.Rays(directions=end - start, origins=start, grid_idx=torch.zeros(R, dtype=torch.int32, device=dev),
                               near=torch.zeros(R, device=dev), far=torch.ones(R, device=dev),
                               encoding=torch.randn(R, shape[3], device=dev, generator=gen))
                for regime, S in (("uniform", 128), ("resampled", 256)):
                    with torch.no_grad():
                        s = lp.ray_samples(rays, S if regime == "uniform" else 64)
                        if regime == "resampled":
                            w = lp.hash_grid_render_samples(rays, s.depths, s.deltas, table, lay, dec, gain=GAIN, return_weights=True,
                                                            with_color=False)[3]
                            s = lp.importance_samples(rays, s.depths, w, S - 64)
                    ups = [torch.randn(R, device=dev, generator=gen), torch.randn(R, device=dev, generator=gen),
                           torch.randn(R, 3, device=dev, generator=gen)]

                    def chain(t, s=s, rays=rays):
                        opacity, color = lp.hash_grid_eval_mlp(s.points, t, rays.grid_idx, lay, dec, rays.encoding, GAIN)
                        return lp.composite_samples(opacity, color, s.depths, s.deltas)

                    def fused(t, s=s, rays=rays):
                        return lp.hash_grid_render_samples(rays, s.depths, s.deltas, t, lay, dec, gain=GAIN)

                    paths = {"chain": chain, "fused": fused}

                    def clear():
                        table.grad = params.grad = None

                    def forward(fn):
                        with torch.no_grad():
                            return fn(table.detach())

                    def fwd_bwd(fn):
                        clear()
                        torch.autograd.backward(fn(table), ups)
                        return table.grad, params.grad

                    results = (R * 5 + R * ((S + 63) // 64)) * 4   # ray_length, -log T, feature [R, 3], chunk_nlt
                    expect = {"forward": results, "forward + backward": results + (table.numel() + params.numel()) * 4}
                    say(f"\nT = 2^{log2_t} ({table.numel() * 4 / mib:.1f} MiB table), decoder {shape[0]}/{shape[1]}/{shape[2]} x {shape[3]}, "
                        f"{R} rays x {S} {regime} samples; the chain's per-sample tensors: {R * S * 28 / mib:.0f} MiB each way")
                    for what, run in (("forward", forward), ("forward + backward", fwd_bwd)):
                        res = {k: [] for k in paths}
                        for key, fn in tuple(paths.items()) * 2:
                            res[key].append(timed(lambda: run(fn), clear, a.reps, a.warmup))
                        for key in paths:
                            for i, r in enumerate(res[key]):
                                say(f"  {what:18s} {key:6s} pass {i}: {r[0]:9.3f} ms [{r[1]:.3f} .. {r[2]:.3f}]  mem +{r[3] / mib:9.1f} MiB")
                        med = {k: statistics.median(r[0] for r in res[k]) for k in paths}
                        mem = {k: max(r[3] for r in res[k]) for k in paths}
                        spread = max(abs(res[k][0][0] - res[k][1][0]) / med[k] for k in paths)
                        say(f"  {what:18s} chain / fused: time {med['chain'] / med['fused']:.2f} x ({med['chain']:.3f} -> {med['fused']:.3f} ms; "
                            f"passes differ by up to {100 * spread:.1f} %), peak memory {mem['chain'] / max(mem['fused'], 1):.2f} x "
                            f"({mem['chain'] / mib:.1f} -> {mem['fused'] / mib:.1f} MiB; fused bound: {expect[what] / mib:.1f} MiB)")
                        if med["fused"] > med["chain"] * (1 + spread):
                            misses.append(f"T = 2^{log2_t}, {shape}, {R} x {S} {regime}, {what} ({med['chain']:.3f} -> {med['fused']:.3f} ms)")
                        got, ref = run(paths["chain"]), run(paths["fused"])
                        worst = max(float((g.detach() - r.detach()).abs().max()) / float(r.detach().abs().max()) for g, r in zip(got, ref))
                        say(f"  {what:18s} chain differs from fused by at most {worst:.2e} of a tensor's max |value| (both fp32)")
    say("\n# fused slower than the chain beyond the spread: " + ("nowhere" if not misses else "; ".join(misses)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

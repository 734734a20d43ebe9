#!/usr/bin/env python
"""Developer benchmark of the plane-field render along rays (lightplane_amd/kplanes.py ``kplanes_render_samples``) on one MI355X.

    python scripts/bench_kplanes_render.py [--rays 65536] [--reps 7] [--warmup 3] [--out profiles/kplanes_render_bench.txt]

``--rays`` rays x 128 uniform samples (``lp.ray_samples``) through a plane field of four scales 64 .. 512 with C in {16, 32} channels,
static and dynamic (m = 150 time vertices, one timestamp per ray), for the decoders 2/2/2 x 32 and 1/1/2 x 64, in ONE process, the paths
alternating:
  chain   lp.kplanes_eval_mlp(samples.points) -> lp.composite_samples: opacity [R, S] and colour [R, S, 3] and their gradients are tensors
  fused   lp.kplanes_render_samples: one launch forward, one backward
for the forward alone (no_grad) and for forward + backward with gradients to the planes and the decoder's parameters.  Protocol and
memory accounting: scripts/bench_hash_points.py (device-event medians, two passes per path, peak above the inputs).  The fused peak is
held against what can be said in advance: the three results + chunk_nlt in the forward, + gradient buffers in forward + backward -- no
[R, S] tensor.  Every row is reported, the ones where the fused op is slower are named at the end.  It needs a GPU and fails without one.
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

GAIN, S = 1.0, 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kplanes_render.py measures on a GPU; there is nothing to fall back to"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# kplanes render bench  {time.strftime('%Y-%m-%d')}  {torch.cuda.get_device_name(0)}  library src {_lib.build_info()['src_hash'][:16]}")
    say(f"# lp.kplanes_render_samples against lp.kplanes_eval_mlp -> lp.composite_samples on the same samples; median of {a.reps} calls "
        f"after {a.warmup} warm-up calls (device events), the paths alternating, two passes each; min / max in brackets; mem = peak bytes "
        "above the inputs")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    misses, mib, R = [], 2.0 ** 20, a.rays
    start, end = (torch.rand(R, 3, device=dev, generator=gen) * 1.8 - 0.9 for _ in range(2))
    for channels in (16, 32):
        for m in (None, 150):
            lay = lp.kplanes_layout((64, 128, 256, 512), m, channels)
            planes = lp.init_kplanes(lay, 1, device=dev, generator=gen).requires_grad_(True)
            times = None if m is None else torch.rand(R, device=dev, generator=gen) * 2 - 1
            for shape in ((2, 2, 2, 32), (1, 1, 2, 64)):
                dec = make_decoder(*shape[:3], lay.out_channels, shape[3], gen, dev)
                params = dec.mlp_params.requires_grad_(True)
                dec = lp.DecoderParams(params, dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
                rays = lp.Rays(directions=end - start, origins=start, grid_idx=torch.zeros(R, dtype=torch.int32, device=dev),
                               near=torch.zeros(R, device=dev), far=torch.ones(R, device=dev),
                               encoding=torch.randn(R, shape[3], device=dev, generator=gen))
                with torch.no_grad():
                    s = lp.ray_samples(rays, S)
                ups = [torch.randn(R, device=dev, generator=gen), torch.randn(R, device=dev, generator=gen),
                       torch.randn(R, 3, device=dev, generator=gen)]

                def chain(p, s=s, rays=rays, times=times, lay=lay, dec=dec):
                    opacity, color = lp.kplanes_eval_mlp(s.points, times, p, rays.grid_idx, lay, dec, rays.encoding, GAIN)
                    return lp.composite_samples(opacity, color, s.depths, s.deltas)

                def fused(p, s=s, rays=rays, times=times, lay=lay, dec=dec):
                    return lp.kplanes_render_samples(rays, times, s.depths, s.deltas, p, lay, dec, gain=GAIN)

                paths = {"chain": chain, "fused": fused}

                def clear():
                    planes.grad = params.grad = None

                def forward(fn):
                    with torch.no_grad():
                        return fn(planes.detach())

                def fwd_bwd(fn):
                    clear()
                    torch.autograd.backward(fn(planes), ups)
                    return planes.grad, params.grad

                results = (R * 5 + R * ((S + 63) // 64)) * 4   # ray_length, -log T, feature [R, 3], chunk_nlt
                expect = {"forward": results, "forward + backward": results + (planes.numel() + params.numel()) * 4}
                say(f"\nC = {channels} x 4 scales, {'static' if m is None else 'dynamic'} ({planes.numel() * 4 / mib:.1f} MiB of planes), decoder "
                    f"{shape[0]}/{shape[1]}/{shape[2]} x {shape[3]}, {R} rays x {S} samples; the chain's per-sample tensors: "
                    f"{R * S * 28 / mib:.0f} MiB each way")
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
                        misses.append(f"C = {channels}, {'static' if m is None else 'dynamic'}, {shape}, {what} "
                                      f"({med['chain']:.3f} -> {med['fused']:.3f} ms)")
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

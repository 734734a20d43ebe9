#!/usr/bin/env python
"""Developer benchmark of the decoder on a plane field at points (lightplane_amd/kplanes.py ``kplanes_eval_mlp``) on one MI355X.

    python scripts/bench_kplanes_points.py [--reps 7] [--warmup 3] [--out profiles/kplanes_points_bench.txt]

The protocol of scripts/bench_hash_points.py.  S = 4 scales 64 .. 512, m = 150 time vertices, C in {16, 32}, static and dynamic, the
decoders 2/2/2 x 32 and 1/1/2 x 64; 2^18 and 2^20 points -- [R, 128, 3] samples along random rays through the box, sorted by depth --
and the 2^20 points permuted (no runs for the scatter to merge), in ONE process, the paths alternating:
  chain   lp.kplanes_encode -> the same decoder from PyTorch ops in fp32 and its autograd: the features [R, N, S C] and their gradient
          are tensors
  fused   lp.kplanes_eval_mlp: one launch forward, one backward
for the forward alone (no_grad) and for forward + backward with gradients to the planes and the decoder's parameters (the training
loop).  Device-event medians over --reps calls after --warmup calls, two passes per path (their spread is the run-to-run spread);
memory is torch.cuda.max_memory_allocated above the inputs, with every gradient buffer counted.  The fused peak is held against what
can be said in advance: the two results in the forward, results + upstream gradients + gradient buffers in forward + backward -- no
[R, N, S C] tensor.  It needs a GPU and fails without one.
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
from scripts.bench_hash_grid import N_PTS  # noqa: E402
from scripts.bench_hash_points import GAIN, make_decoder, timed, torch_decoder  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kplanes_points.py measures on a GPU; there is nothing to fall back to"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# kplanes points bench  {time.strftime('%Y-%m-%d')}  {torch.cuda.get_device_name(0)}  library src {_lib.build_info()['src_hash'][:16]}")
    say(f"# lp.kplanes_eval_mlp against lp.kplanes_encode -> the same decoder from PyTorch ops; median of {a.reps} calls after "
        f"{a.warmup} warm-up calls (device events), the paths alternating, two passes each; min / max in brackets; mem = peak bytes above "
        "the inputs")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    misses, mib = [], 2.0 ** 20
    for channels in (16, 32):
        for m in (None, 150):
            lay = lp.kplanes_layout((64, 128, 256, 512), m, channels)
            planes = lp.init_kplanes(lay, 1, device=dev, generator=gen).requires_grad_(True)
            kind = "static" if m is None else "dynamic"
            for shape in ((2, 2, 2, 32), (1, 1, 2, 64)):
                dec = make_decoder(*shape[:3], lay.out_channels, shape[3], gen, dev)
                params = dec.mlp_params.requires_grad_(True)
                dec = lp.DecoderParams(params, dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
                for n_points, permuted in ((1 << 18, False), (1 << 20, False), (1 << 20, True)):
                    R = n_points // N_PTS
                    start, end = (torch.rand(R, 1, 3, device=dev, generator=gen) * 1.8 - 0.9 for _ in range(2))
                    pts = start + torch.rand(R, N_PTS, 1, device=dev, generator=gen).sort(dim=1).values * (end - start)
                    if permuted:
                        pts = pts.reshape(-1, 3)[torch.randperm(n_points, device=dev, generator=gen)].reshape(R, N_PTS, 3).contiguous()
                    times = None if m is None else torch.rand(R, device=dev, generator=gen) * 2 - 1
                    gidx = torch.zeros(R, dtype=torch.int64, device=dev)
                    enc = torch.randn(R, shape[3], device=dev, generator=gen)
                    u_op, u_col = torch.randn(R, N_PTS, device=dev, generator=gen), torch.randn(R, N_PTS, 3, device=dev, generator=gen)
                    paths = {"chain": lambda t, p=pts, ts=times, e=enc, g=gidx: torch_decoder(lp.kplanes_encode(p, ts, t, g, lay), dec, params, e),
                             "fused": lambda t, p=pts, ts=times, e=enc, g=gidx: lp.kplanes_eval_mlp(p, ts, t, g, lay, dec, e, GAIN)}

                    def clear():
                        planes.grad = params.grad = None

                    def forward(fn):
                        with torch.no_grad():
                            return fn(planes.detach())

                    def fwd_bwd(fn):
                        clear()
                        op, col = fn(planes)
                        ((op * u_op).sum() + (col * u_col).sum()).backward()
                        return planes.grad, params.grad

                    results = n_points * 4 * 4   # opacity + 3 colours
                    expect = {"forward": results,
                              "forward + backward": 2 * results + (planes.numel() + params.numel()) * 4}   # + upstream gradients + gradient buffers
                    row = (f"C = {channels} {kind} ({planes.numel() * 4 / mib:.1f} MiB planes), decoder {shape[0]}/{shape[1]}/{shape[2]} x "
                           f"{shape[3]}, {n_points} points{' permuted' if permuted else f' = {R} rays x {N_PTS}'}")
                    say(f"\n{row}; features [R, N, S C]: {n_points * lay.out_channels * 4 / mib:.0f} MiB")
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
                            f"({mem['chain'] / mib:.1f} -> {mem['fused'] / mib:.1f} MiB; fused bound: {expect[what] / mib:.1f} MiB + the loss's "
                            "own products in forward + backward)")
                        if med["fused"] > med["chain"] * (1 + spread):
                            misses.append(f"{row}, {what} ({med['chain']:.3f} -> {med['fused']:.3f} ms)")
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

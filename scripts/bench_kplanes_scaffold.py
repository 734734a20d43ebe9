#!/usr/bin/env python
"""Developer benchmark of the plane-field scaffold (lightplane_amd/kplanes_scaffold.py, csrc/lp_kplanes_scaffold.hip) on one MI355X.

    python scripts/bench_kplanes_scaffold.py [--reps 10] [--warmup 2] [--sizes 128,256] [--out profiles/kplanes_scaffold_bench.txt]

(profiles/kplanes_scaffold_bench.txt is recorded with these defaults.)

The field of the README's K-Planes rows: S = 4 scales of 64, 128, 256 and 512 vertices per axis, 150 vertices on t (or static),
C = 32 and 16 channels, decoders 2/2 x 32 and 1/1 x 64, one scene, lattices of 128^3 and 256^3 points, dilate = 2, static / T = 1 /
T = 8 timestamps, in ONE process, the two paths alternating on the same planes:
  composed  what a user had to write: the explicit lattice points [1, D H W, 3], lp.kplanes_eval_mlp_opacity_only once per timestamp,
            a running torch.maximum, max_pool3d(2 r + 1) > threshold
  fused     lp.kplanes_calculate_scaffold
Device-event medians over --reps calls after --warmup calls, two passes per path (their spread is the run-to-run spread); memory is
torch.cuda.max_memory_allocated above what was allocated before the calls (the planes, the decoder and the timestamps: the inputs).
The threshold is the median of the fused opacity lattice, so neither path is trivial and the early exit of the time loop is neither
always nor never taken; the script checks that the two paths agree on all but a few lattice points (fp32 round-off at the threshold)
and exits non-zero otherwise.  It needs a GPU and fails without one.
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

SPATIAL, TEMPORAL, DILATE, GAIN = (64, 128, 256, 512), 150, 2, 1.0


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


def composed(planes, lay, dec, n, times, threshold):
    lin = torch.linspace(0, 1, n, device=planes.device) * 2 - 1
    zz, yy, xx = torch.meshgrid(lin, lin, lin, indexing="ij")
    pts = torch.stack([xx, yy, zz], -1).reshape(1, -1, 3)
    idx = torch.zeros(1, dtype=torch.int32, device=planes.device)
    best = None
    for t in [None] if times is None else times.split(1):
        op = lp.kplanes_eval_mlp_opacity_only(pts, t, planes, idx, lay, dec, GAIN)
        best = op if best is None else torch.maximum(best, op)
    pooled = torch.nn.functional.max_pool3d(best.view(1, n, n, n), 2 * DILATE + 1, stride=1, padding=DILATE)
    return (pooled > threshold).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", type=lambda v: tuple(int(x) for x in v.split(",")), default=(128, 256))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kplanes_scaffold.py measures on a GPU; there is nothing to fall back to"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# kplanes_scaffold bench  {time.strftime('%Y-%m-%d')}  {torch.cuda.get_device_name(0)}  library src {_lib.build_info()['src_hash'][:16]}")
    say(f"# lp.kplanes_calculate_scaffold (dilate {DILATE}) against lattice points -> kplanes_eval_mlp_opacity_only per timestamp -> running "
        f"maximum -> max_pool3d > t; median of {a.reps} calls after {a.warmup} warm-up calls (device events), the paths alternating, two "
        "passes each; min / max in brackets; mem = peak bytes above the inputs")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    slower, differ = [], []
    for n in a.sizes:
        for channels in (32, 16):
            for n_t, n_o, hidden in ((2, 2, 32), (1, 1, 64)):
                for T in (0, 1, 8):   # 0: the static layout
                    lay = lp.kplanes_layout(SPATIAL, TEMPORAL if T else None, channels)
                    planes = (0.5 + torch.rand(1, lay.rows, channels, device=dev, generator=gen)) * (
                        torch.randint(0, 2, (1, 1, channels), device=dev, generator=gen) * 2 - 1)
                    dec = lp.init_decoder_params(dev, n_o, n_t, 2, input_chn=lay.out_channels, hidden_chn=hidden, color_chn=3)
                    dec = lp.DecoderParams(torch.randn(dec.mlp_params.shape, device=dev, generator=gen) * (2.0 / hidden) ** 0.5,
                                           dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
                    times = torch.linspace(-0.9, 0.9, T, device=dev) if T else None
                    size = [1, n, n, n]
                    thr = float(lp.kplanes_scaffold_opacity(planes, lay, dec, size, times=times, gain=GAIN).median())
                    run = {"composed": lambda: composed(planes, lay, dec, n, times, thr),
                           "fused": lambda: lp.kplanes_calculate_scaffold(planes, lay, dec, size, times=times, gain=GAIN, threshold=thr,
                                                                          dilate_scaffold=DILATE)}
                    tag = f"{n}^3, C = {channels}, {n_t}/{n_o} x {hidden}, " + (f"T = {T}" if T else "static")
                    bad = int((run["composed"]() != run["fused"]()).sum())
                    res = {"composed": [], "fused": []}
                    for key in ("composed", "fused") * 2:
                        res[key].append(timed(run[key], a.reps, a.warmup))
                    for key in res:
                        for i, r in enumerate(res[key]):
                            say(f"  {tag:42s} {key:8s} pass {i}: {r[0]:9.3f} ms [{r[1]:.3f} .. {r[2]:.3f}]  mem +{r[3] / 2 ** 20:9.1f} MiB")
                    med = {k: statistics.median(r[0] for r in res[k]) for k in res}
                    mem = {k: max(r[3] for r in res[k]) for k in res}
                    spread = max(abs(res[k][0][0] - res[k][1][0]) / med[k] for k in res)
                    say(f"  {tag:42s} composed / fused: time {med['composed'] / med['fused']:.2f} x ({med['composed']:.3f} -> "
                        f"{med['fused']:.3f} ms; passes differ by up to {100 * spread:.1f} %), peak memory "
                        f"{mem['composed'] / 2 ** 20:.1f} -> {mem['fused'] / 2 ** 20:.1f} MiB; {bad} of {n ** 3} points differ")
                    if med["fused"] > med["composed"] * (1 + spread):
                        slower.append(f"{tag} ({med['composed']:.3f} -> {med['fused']:.3f} ms)")
                    if bad > 1e-4 * n ** 3:
                        differ.append(tag)
                    del planes
    say("\n# fused slower than the composition beyond the spread: " + ("nowhere" if not slower else "; ".join(slower)))
    say("# the two paths differ on more than 1e-4 of the lattice: " + ("nowhere" if not differ else "; ".join(differ)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())

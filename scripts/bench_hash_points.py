#!/usr/bin/env python
"""Developer benchmark of the decoder on a hash grid at points (lightplane_amd/hash_grid.py ``hash_grid_eval_mlp``) on one MI355X.

    python scripts/bench_hash_points.py [--reps 7] [--warmup 3] [--out profiles/hash_points_bench.txt]

At 2^18 and 2^20 points -- [R, 128, 3] samples along random rays through the box, sorted by depth -- with L = 16 levels of F = 2
features from 16 to 2048, for a 2^19-entry and a 2^14-entry table and the decoders 2/2/2 x 32 and 1/1/2 x 64, in ONE process, the paths
alternating:
  chain   lp.hash_grid_encode -> the same decoder from PyTorch ops in fp32 (matmul + bias, ReLU between layers; softplus / sigmoid) and
          its autograd: the features [R, N, L F] and their gradient are tensors
  fused   lp.hash_grid_eval_mlp: one launch forward, one backward
for the forward alone (no_grad) and for forward + backward with gradients to the table and the decoder's parameters (the training
loop).  Device-event medians over --reps calls after --warmup calls, two passes per path (their spread is the run-to-run spread);
memory is torch.cuda.max_memory_allocated above the inputs (the gradients of earlier calls are dropped before the baseline is taken,
so every buffer a call allocates counts).  The fused peak is held against what can be said in advance: the two results in the
forward, results + upstream gradients + gradient buffers in forward + backward -- no [R, N, L F] tensor.  The fused path is
point-major (a wave walks all L level tables) where the stand-alone encoding is level-major; the T = 2^19
rows show what that costs.  It needs a GPU and fails without one.
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
from lightplane_amd.params import int_list_of  # noqa: E402
from scripts.bench_hash_grid import N_PTS  # noqa: E402

GAIN = 1.0


def timed(fn, clear, reps, warmup):
    """(median ms, min ms, max ms, peak bytes above the inputs) of fn(); clear() drops what earlier calls left allocated -- the
    gradients -- before the baseline is taken, so that every buffer a call allocates counts"""
    for _ in range(warmup):
        fn()
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
    peak = torch.cuda.max_memory_allocated() - base
    clear()
    return statistics.median(ms), min(ms), max(ms), peak


def make_decoder(n_t, n_o, n_c, width, hidden, gen, dev):
    """DecoderParams with N(0, 2 / fan-in) weights in the flat trunk | opacity | colour layout"""
    def mlp(n, d_in, d_out):
        dims = [d_in] + [hidden] * (n - 1) + [d_out]
        return ([torch.randn(i, o, device=dev, generator=gen) * (2.0 / i) ** 0.5 for i, o in zip(dims[:-1], dims[1:])],
                [torch.zeros(o, device=dev) for o in dims[1:]])
    wt, bt = mlp(n_t, width, hidden)
    wo, bo = mlp(n_o, hidden, 1)
    wc, bc = mlp(n_c, hidden, 3)
    flat, nt, no, nc = lp.flatten_decoder_params(wt, bt, wo, bo, wc, bc, True)
    return lp.DecoderParams(flat, nt, no, nc, 3)


def torch_decoder(feat, dec, params, enc):
    """the decoder of hash_grid_eval_mlp on a feature tensor, from PyTorch ops"""
    def run(x, dims, off):
        pairs = list(zip(dims[:-1], dims[1:]))
        b_off = off + sum(i * o for i, o in pairs)   # (an MLP's weights come first, then its biases)
        for l, (i, o) in enumerate(pairs):
            x = x @ params[off:off + i * o].view(i, o) + params[b_off:b_off + o]
            off, b_off = off + i * o, b_off + o
            if l < len(pairs) - 1:
                x = torch.relu(x)
        return x, b_off
    dt, do, dc = (int_list_of(v) for v in (dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color))
    t, off = run(feat, dt, 0)
    t = torch.relu(t)
    raw, off = run(t, do, off)
    craw, _ = run(t + enc[:, None], dc, off)
    return GAIN * torch.nn.functional.softplus(raw[..., 0]), torch.sigmoid(craw[..., :3])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_hash_points.py measures on a GPU; there is nothing to fall back to"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# hash points bench  {time.strftime('%Y-%m-%d')}  {torch.cuda.get_device_name(0)}  library src {_lib.build_info()['src_hash'][:16]}")
    say(f"# lp.hash_grid_eval_mlp against lp.hash_grid_encode -> the same decoder from PyTorch ops; median of {a.reps} calls after "
        f"{a.warmup} warm-up calls (device events), the paths alternating, two passes each; min / max in brackets; mem = peak bytes above "
        "the inputs")
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
            for n_points in (1 << 18, 1 << 20):
                R = n_points // N_PTS
                start, end = (torch.rand(R, 1, 3, device=dev, generator=gen) * 1.8 - 0.9 for _ in range(2))
                pts = start + torch.rand(R, N_PTS, 1, device=dev, generator=gen).sort(dim=1).values * (end - start)
                gidx = torch.zeros(R, dtype=torch.int64, device=dev)
                enc = torch.randn(R, shape[3], device=dev, generator=gen)
                u_op, u_col = torch.randn(R, N_PTS, device=dev, generator=gen), torch.randn(R, N_PTS, 3, device=dev, generator=gen)
                paths = {"chain": lambda t, p=pts, e=enc, g=gidx: torch_decoder(lp.hash_grid_encode(p, t, g, lay), dec, params, e),
                         "fused": lambda t, p=pts, e=enc, g=gidx: lp.hash_grid_eval_mlp(p, t, g, lay, dec, e, GAIN)}

                def clear():
                    table.grad = params.grad = None

                def forward(fn):
                    with torch.no_grad():
                        return fn(table.detach())

                def fwd_bwd(fn):
                    clear()
                    op, col = fn(table)
                    ((op * u_op).sum() + (col * u_col).sum()).backward()
                    return table.grad, params.grad

                results = n_points * 4 * 4   # opacity + 3 colours
                expect = {"forward": results,
                          "forward + backward": 2 * results + (table.numel() + params.numel()) * 4}   # + upstream gradients + gradient buffers
                say(f"\nT = 2^{log2_t} ({table.numel() * 4 / mib:.1f} MiB table), decoder {shape[0]}/{shape[1]}/{shape[2]} x {shape[3]}, "
                    f"{n_points} points = {R} rays x {N_PTS}; features [R, N, L F]: {n_points * lay.channels * 4 / mib:.0f} MiB")
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
                    say(f"  {what:18s} chain / fused: time {med['chain'] / med['fused']:.2f} x ({med['chain']:.3f} -> {med['fused']:.3f} ms; passes "
                        f"differ by up to {100 * spread:.1f} %), peak memory {mem['chain'] / max(mem['fused'], 1):.2f} x "
                        f"({mem['chain'] / mib:.1f} -> {mem['fused'] / mib:.1f} MiB; fused bound: {expect[what] / mib:.1f} MiB + the loss's own "
                        "products in forward + backward)")
                    if med["fused"] > med["chain"] * (1 + spread):
                        misses.append(f"T = 2^{log2_t}, {shape}, {n_points} points, {what} ({med['chain']:.3f} -> {med['fused']:.3f} ms)")
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

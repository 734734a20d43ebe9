#!/usr/bin/env python
"""Developer benchmark of the distortion and the interlevel loss (lightplane_amd/ray_losses.py) on one MI355X.

    python scripts/bench_ray_losses.py [--reps 5] [--warmup 2] [--out profiles/ray_losses_bench.txt]

At 65 536 rays, S = 128 samples (and P = 128 proposal samples) per ray, in ONE process, the paths alternating:
  torch   the O(S) composition from PyTorch ops and its autograd -- distortion: two ``cumsum`` (of ``w`` and ``w d``) and
          ``2 sum w_i (d_i A_{i-1} - B_{i-1}) + sum w_i^2 delta_i / 3``; interlevel: the edges, ``searchsorted`` of the target edges in the
          proposal's, ``cumsum`` of the proposal weights, two ``gather`` and the ratio
  pairs   (distortion only, at 4 096 rays: the batch its ``[R, S, S]`` tensors fit comfortably) ``sum_ij w_i w_j |d_i - d_j|`` as written
  fused   lp.distortion_loss / lp.interlevel_loss
for the forward alone (no_grad) and for forward + backward (distortion: gradients to weights, depths and deltas; interlevel: to the
proposal weights).  Protocol of scripts/bench_compositing.py: device-event medians over --reps calls after --warmup calls, two passes
per path; memory is torch.cuda.max_memory_allocated above what was allocated before the calls (results and gradients included).  The
fused rows also give the fraction of the achievable HBM rate (6.29 TB/s: the measured float4 copy rate of the chip) that the
algorithmic bytes imply: every input read once per launch, every result and gradient written once.
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

R, S, P, R_PAIRS = 65536, 128, 128, 4096
HBM_BYTES_PER_S = 6.29e12
EPS = 1e-7


def timed(fn, reps, warmup, clear):
    """(median ms, min ms, max ms, peak bytes above the starting allocation) of fn()"""
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
        clear()
    return statistics.median(ms), min(ms), max(ms), torch.cuda.max_memory_allocated() - base


def torch_distortion(w, d, delta):
    """the O(S) composition a user would write: prefix sums of w and of w d"""
    wd = w * d
    a_before = torch.cumsum(w, 1) - w
    b_before = torch.cumsum(wd, 1) - wd
    return 2 * (w * (d * a_before - b_before)).sum(-1) + (w * w * delta).sum(-1) / 3


def torch_distortion_pairs(w, d, delta):
    return (w[:, :, None] * w[:, None, :] * (d[:, :, None] - d[:, None, :]).abs()).sum((1, 2)) + (w * w * delta).sum(-1) / 3


def torch_interlevel(w, d, pw, pd):
    with torch.no_grad():
        e = torch.cat([d[:, :1], 0.5 * (d[:, :-1] + d[:, 1:]), d[:, -1:]], 1)
        eh = torch.cat([pd[:, :1], 0.5 * (pd[:, :-1] + pd[:, 1:]), pd[:, -1:]], 1)
        n = torch.searchsorted(eh, e, right=True)
        lo, hi = (n[:, :-1] - 1).clamp(min=0), n[:, 1:].clamp(max=pd.shape[1])
    C = torch.nn.functional.pad(torch.cumsum(pw, 1), (1, 0))
    x = (w - (C.gather(1, hi) - C.gather(1, lo))).clamp(min=0)
    return (x * x / (w + EPS)).sum(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ray_losses.py measures on a GPU; there is nothing to fall back to"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# ray losses bench  {time.strftime('%Y-%m-%d')}  {torch.cuda.get_device_name(0)}  library src {_lib.build_info()['src_hash'][:16]}")
    say(f"# lp.distortion_loss / lp.interlevel_loss against the same losses composed from PyTorch ops (and their autograd); median of "
        f"{a.reps} calls after {a.warmup} warm-up calls (device events), the paths alternating, two passes each; min / max in brackets; "
        "mem = peak bytes above the start")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)

    def rows(n, s):
        deltas = torch.rand(n, s, device=dev, generator=gen) * 0.05 + 0.01
        return 0.5 + torch.cumsum(deltas, -1), deltas

    def bump(n, s, height, width):  # the weights of a ray that meets a surface, on a floor of 1e-4
        centre = torch.rand(n, 1, device=dev, generator=gen) * s
        return height * torch.exp(-0.5 * ((torch.arange(s, device=dev)[None] - centre) / width) ** 2) + 1e-4

    misses = []

    def compare(title, paths, inputs, n_grad, fwd_bytes, bwd_bytes, names):
        """``paths``: name -> fn(*inputs); the first ``n_grad`` inputs get gradients; the last path is the fused one"""
        leaves = [t.clone().requires_grad_(True) for t in inputs[:n_grad]]
        up = torch.rand(inputs[0].shape[0], device=dev, generator=gen) + 0.5

        def clear():
            for t in leaves:
                t.grad = None

        def forward(fn):
            with torch.no_grad():
                return (fn(*inputs),)

        def fwd_bwd(fn):
            clear()
            (fn(*leaves, *inputs[n_grad:]) * up).sum().backward()
            return [t.grad for t in leaves]

        say(f"\n{title}")
        for what, run, nbytes in (("forward", forward, fwd_bytes), ("forward + backward", fwd_bwd, fwd_bytes + bwd_bytes)):
            res = {k: [] for k in paths}
            for key, fn in tuple(paths.items()) * 2:
                res[key].append(timed(lambda: run(fn), a.reps, a.warmup, clear))
            for key in paths:
                for i, r in enumerate(res[key]):
                    say(f"  {what:22s} {key:8s} pass {i}: {r[0]:9.3f} ms [{r[1]:.3f} .. {r[2]:.3f}]  mem +{r[3] / 2 ** 20:9.1f} MiB")
            med = {k: statistics.median(r[0] for r in res[k]) for k in paths}
            mem = {k: max(r[3] for r in res[k]) for k in paths}
            tf, mf = med["fused"], mem["fused"]
            for key in paths:
                if key == "fused":
                    continue
                say(f"  {what:22s} {key} / fused: time {med[key] / tf:.2f} x ({med[key]:.3f} -> {tf:.3f} ms), peak memory "
                    f"{mem[key] / max(mf, 1):.2f} x ({mem[key] / 2 ** 20:.1f} -> {mf / 2 ** 20:.1f} MiB)")
                if tf > med[key]:
                    misses.append(f"{title.split(',')[0]} {what} against {key}: not faster ({med[key]:.3f} -> {tf:.3f} ms)")
            say(f"  {what:22s} fused: {nbytes / 2 ** 20:.0f} MiB of algorithmic traffic = {nbytes / (tf * 1e-3) / HBM_BYTES_PER_S:.2f} of the "
                "achievable HBM rate")
            ref = run(paths["fused"])
            ref = [t.detach().clone() for t in ref]
            for key, fn in paths.items():
                if key == "fused":
                    continue
                got = run(fn)
                labels = ("loss",) if what == "forward" else names
                diffs = ", ".join(f"{n} {float((p - q).abs().max()) / max(float(q.abs().max()), 1e-30):.2e}" for n, p, q in zip(labels, got, ref))
                say(f"  {what:22s} {key} differs from fused by at most (of a tensor's max |value|; both fp32): {diffs}")
        clear()

    depths, deltas = rows(R, S)
    weights = bump(R, S, 0.25, 2.0)
    row = 4 * R * S
    compare(f"distortion_loss, {R} rays, S = {S} samples per ray", {"torch": torch_distortion, "fused": lp.distortion_loss},
            (weights, depths, deltas), 3, 3 * row + 4 * R, 3 * row + 4 * R + 3 * row, ("d weights", "d depths", "d deltas"))
    n = R_PAIRS
    compare(f"distortion_loss, {n} rays, S = {S}: against the pairwise [R, S, S] form",
            {"pairs": torch_distortion_pairs, "torch": torch_distortion, "fused": lp.distortion_loss},
            (weights[:n].contiguous(), depths[:n].contiguous(), deltas[:n].contiguous()), 3, (3 * row + 4 * R) * n // R,
            (6 * row + 4 * R) * n // R, ("d weights", "d depths", "d deltas"))
    # interlevel: a fine march (S samples, a sharp bump) against a coarse one (P samples over the same span, a flatter and lower bump)
    run_sum = rows(R, P)[0] - 0.5
    p_depths = depths[:, :1] + run_sum / run_sum[:, -1:] * (depths[:, -1:] - depths[:, :1])
    p_weights = bump(R, P, 0.1, 4.0)
    prow = 4 * R * P
    compare(f"interlevel_loss, {R} rays, S = {S} target + P = {P} proposal samples per ray",
            {"torch": lambda pw, w, d, pd: torch_interlevel(w, d, pw, pd), "fused": lambda pw, w, d, pd: lp.interlevel_loss(w, d, pw, pd, eps=EPS)},
            (p_weights, weights, depths, p_depths), 1, 2 * row + 2 * prow + 4 * R, 2 * row + 2 * prow + 4 * R + prow, ("d proposal_weights",))
    say("\n# fused slower than a PyTorch composition: " + ("nowhere" if not misses else "; ".join(misses)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

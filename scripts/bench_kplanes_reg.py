#!/usr/bin/env python
"""Developer benchmark of the K-Planes regularisers (lightplane_amd/regularizers.py, csrc/lp_kplanes_reg.hip) on one MI355X.

    python scripts/bench_kplanes_reg.py [--reps 9] [--warmup 3] [--out profiles/kplanes_reg_bench.txt]

The dynamic field of the README's K-Planes rows: S = 4 scales of 64, 128, 256 and 512 vertices per axis, 150 vertices on t, C = 32 and
16 channels, B = 1 and 2 scenes, in ONE process, the paths alternating on the same planes:
  torch   the three terms as a user would compose them: 24 slices ``planes[:, off : off + n_u * n_v].view(B, n_v, n_u, C)``, differences,
          ``abs`` / ``square``, ``mean``, and their autograd
  fused   lp.kplanes_regularizers (value; value + gradient through autograd) and lp.add_kplanes_reg_grad_ (the accumulate in one sweep;
          its torch twin is value + gradient followed by ``grad.add_``)
Device-event medians over --reps calls after --warmup calls, two passes per path (their spread is the run-to-run spread); memory is
torch.cuda.max_memory_allocated above what was allocated before the calls.  The script holds the fused paths to their memory bound
itself and exits non-zero where it is missed: value + gradient allocates the workspace (lp.kplanes_reg_workspace_bytes) and one
grad_planes, the accumulate the workspace only (plus 1 MiB per tensor for the caching allocator, which hands out a whole block where
splitting it would leave less).  GB/s is the bytes the op has to move -- the planes once per sweep, the gradient written once (and read
once by the accumulate) -- over the CALL's time (launches and allocation included, not a kernel time), beside its share of the nominal
8 TB/s of HBM.  It needs a GPU and fails without one.
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

SPATIAL, TEMPORAL, P = (64, 128, 256, 512), 150, 2
ALLOC_SLACK = 1 << 20   # the caching allocator does not split a block when the remainder is under 1 MiB
HBM_BYTES_PER_S = 8e12


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
        release()
    return statistics.median(ms), min(ms), max(ms), torch.cuda.max_memory_allocated() - base


def torch_terms(planes, lay, p=P):
    """the three terms as a user would compose them"""
    phi = torch.abs if p == 1 else torch.square
    tv = smooth = l1 = 0.0
    for s in range(lay.n_scales):
        for j in range(lay.n_planes):
            n_u, n_v = lay.spatial[s], lay.spatial[s] if j < 3 else lay.temporal[s]
            X = planes[:, lay.offsets[s][j]:lay.offsets[s][j] + n_u * n_v].view(planes.shape[0], n_v, n_u, -1)
            tv = tv + phi(X[:, :, 1:] - X[:, :, :-1]).mean()
            if j < 3:
                tv = tv + phi(X[:, 1:] - X[:, :-1]).mean()
            else:
                smooth = smooth + (X[:, 2:] - 2 * X[:, 1:-1] + X[:, :-2]).square().mean()
                l1 = l1 + (1 - X).abs().mean()
    return torch.stack([tv, smooth, l1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kplanes_reg.py measures on a GPU; there is nothing to fall back to"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# kplanes_reg bench  {time.strftime('%Y-%m-%d')}  {torch.cuda.get_device_name(0)}  library src {_lib.build_info()['src_hash'][:16]}")
    say(f"# lp.kplanes_regularizers / lp.add_kplanes_reg_grad_ (p = {P}) against the same three terms composed from slices, differences and "
        f"means (and their autograd); median of {a.reps} calls after {a.warmup} warm-up calls (device events), the paths alternating, two "
        "passes each; min / max in brackets; mem = peak bytes above the start, bound = what the fused path may allocate; GB/s = needed "
        "bytes over the call's time (share of the nominal 8 TB/s)")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    up = torch.tensor([1e-3, 1e-2, 1e-4], device=dev)
    weights = tuple(float(v) for v in up)
    slower, missed = [], []
    for channels in (32, 16):
        for batch in (1, 2):
            lay = lp.kplanes_layout(SPATIAL, TEMPORAL, channels)
            planes = (torch.rand(batch, lay.rows, channels, device=dev, generator=gen) * 0.4 + 0.8).requires_grad_(True)
            acc = torch.randn(planes.shape, device=dev, generator=gen) * 1e-3   # the gradient the accumulate adds to
            plane_bytes, ws = planes.numel() * 4, lp.kplanes_reg_workspace_bytes(lay, batch)

            def value(fused):
                with torch.no_grad():
                    return lp.kplanes_regularizers(planes, lay, p=P) if fused else torch_terms(planes, lay)

            def value_grad(fused):
                planes.grad = None
                (lp.kplanes_regularizers(planes, lay, p=P) if fused else torch_terms(planes, lay)).backward(up)
                return planes.grad

            def accumulate(fused):
                if fused:
                    lp.add_kplanes_reg_grad_(planes.detach(), acc, lay, weights=weights, p=P)
                else:
                    acc.add_(value_grad(False))
                return acc

            say(f"\nC = {channels}, B = {batch} ({lay.n_planes} planes x {lay.n_scales} scales, {plane_bytes / 2 ** 20:.1f} MiB of planes, "
                f"workspace {ws} bytes)")
            #   what, the call, planes-sized tensors the fused op has to move, what the fused op may allocate
            for what, run, moved, bound in (("value", value, 1, ws + 2 * ALLOC_SLACK),
                                            ("value + gradient", value_grad, 3, ws + plane_bytes + 3 * ALLOC_SLACK),
                                            ("fused accumulate", accumulate, 3, ws + 2 * ALLOC_SLACK)):
                res = {"torch": [], "fused": []}
                for key in ("torch", "fused") * 2:
                    res[key].append(timed(lambda: run(key == "fused"), a.reps, a.warmup, lambda: setattr(planes, "grad", None)))
                for key in res:
                    for i, r in enumerate(res[key]):
                        say(f"  {what:17s} {key:6s} pass {i}: {r[0]:9.3f} ms [{r[1]:.3f} .. {r[2]:.3f}]  mem +{r[3] / 2 ** 20:9.1f} MiB")
                med = {k: statistics.median(r[0] for r in res[k]) for k in res}
                mem = {k: max(r[3] for r in res[k]) for k in res}
                spread = max(abs(res[k][0][0] - res[k][1][0]) / med[k] for k in res)
                rate = moved * plane_bytes / (med["fused"] * 1e-3)
                ok = mem["fused"] <= bound
                say(f"  {what:17s} torch / fused: time {med['torch'] / med['fused']:.2f} x ({med['torch']:.3f} -> {med['fused']:.3f} ms; passes differ "
                    f"by up to {100 * spread:.1f} %), peak memory {mem['torch'] / max(mem['fused'], 1):.2f} x ({mem['torch'] / 2 ** 20:.1f} -> "
                    f"{mem['fused'] / 2 ** 20:.1f} MiB; bound {bound / 2 ** 20:.1f} MiB: {'met' if ok else 'MISSED'}); fused moves "
                    f"{moved} x planes at {rate / 1e9:.0f} GB/s ({100 * rate / HBM_BYTES_PER_S:.0f} % of 8 TB/s)")
                tag = f"C = {channels}, B = {batch}, {what}"
                if not ok:
                    missed.append(tag)
                if med["fused"] > med["torch"] * (1 + spread):
                    slower.append(f"{tag} ({med['torch']:.3f} -> {med['fused']:.3f} ms)")
            with torch.no_grad():
                got, ref = torch_terms(planes, lay), lp.kplanes_regularizers(planes, lay, p=P)
            say(f"  terms torch {[f'{float(v):.6e}' for v in got]} fused {[f'{float(v):.6e}' for v in ref]}")
            del planes, acc
    say("\n# fused slower than the PyTorch composition beyond the spread: " + ("nowhere" if not slower else "; ".join(slower)))
    say("# memory bound of the fused paths missed: " + ("nowhere" if not missed else "; ".join(missed)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python
"""Developer benchmark of rendering at caller-given depths (lightplane_amd/render_samples.py) on one MI355X.

    python scripts/bench_render_samples.py [--reps 10] [--warmup 3] [--out profiles/render_samples_bench.txt]

In ONE process, the two paths alternating, two passes each:
  chain   lp.lightplane_eval_mlp on the points the sample op wrote, then lp.composite_samples (what the march in pieces did before)
  fused   lp.render_samples on the depths and deltas of the same samples
for the forward alone (no_grad) and for forward + backward with gradients to the planes, the decoder's parameters and the ray
encoding, upstream gradients on all three results.  Workloads: 65 536 and 4 096 rays; the 2/2/2 x 32 decoder on a 64^2 x 16 triplane and
the 1/1/2 x 64 decoder on a 128^2 x 32 triplane; S = 128 uniform samples (lp.ray_samples) and S = 256 samples from lp.importance_samples
(128 coarse + 128 new, drawn from the weights of the coarse pass).  The sample ops are outside the timed window on both paths.

Device-event medians over --reps calls (eight times as many at 4 096 rays, so that a window is not a few milliseconds) after --warmup
calls; min / max in brackets; memory is torch.cuda.max_memory_allocated above what was allocated before the calls (results and gradients
included).  The spread of a path is the difference of its two passes' medians; a fused row slower than the chain by more than the
chain's own spread is listed at the end.  Whole-call times: no kernel-level rate or share of peak is derived here.
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

SCENES = {"2/2/2x32 on triplane 64^2x16": ((2, 2, 2, 32), 64, 16), "1/1/2x64 on triplane 128^2x32": ((1, 1, 2, 64), 128, 32)}
RAYS = (65536, 4096)
GAIN = 1.0


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
    return statistics.median(ms), min(ms), max(ms), torch.cuda.max_memory_allocated() - base


def random_rays(n, gen, dev, enc_dim):
    """cameras on a sphere of radius 2.5 looking at points of the unit ball (examples/fit_synthetic_scene.py)"""
    o = torch.randn(n, 3, device=dev, generator=gen)
    o = 2.5 * o / o.norm(dim=-1, keepdim=True)
    tgt = torch.randn(n, 3, device=dev, generator=gen)
    tgt = 0.8 * tgt / tgt.norm(dim=-1, keepdim=True) * torch.rand(n, 1, device=dev, generator=gen) ** (1 / 3)
    d = tgt - o
    d = d / d.norm(dim=-1, keepdim=True)
    return lp.Rays(directions=d, origins=o, grid_idx=torch.zeros(n, dtype=torch.int32, device=dev), near=torch.full((n,), 1.2, device=dev),
                   far=torch.full((n,), 3.8, device=dev), encoding=torch.randn(n, enc_dim, device=dev, generator=gen).requires_grad_(True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_render_samples.py measures on a GPU; there is nothing to fall back to"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# render_samples bench  {time.strftime('%Y-%m-%d')}  {torch.cuda.get_device_name(0)}  library src {_lib.build_info()['src_hash'][:16]}")
    say("# lp.render_samples (fused) against lp.lightplane_eval_mlp + lp.composite_samples on the same samples (chain); median of "
        f"{a.reps} calls (x 8 at 4 096 rays) after {a.warmup} warm-up calls (device events), the two paths alternating, two passes each; "
        "min / max in brackets; mem = peak bytes above the start; whole-call times")
    dev = torch.device("cuda:0")
    slower, more_memory = [], []
    for sname, ((n_t, n_o, n_c, hidden), res, chn) in SCENES.items():
        torch.manual_seed(0)
        mod = lp.LightplaneRenderer(num_samples=128, color_chn=3, grid_chn=chn, mlp_hidden_chn=hidden, mlp_n_layers_trunk=n_t,
                                    mlp_n_layers_opacity=n_o, mlp_n_layers_color=n_c, opacity_init_bias=-1.0,
                                    ray_embedding_num_harmonics=None).to(dev)
        with torch.no_grad():
            mod.mlp_params.mul_(3.0)
        dec = mod.get_decoder_params()
        gen = torch.Generator(device=dev).manual_seed(0)
        grids = [(0.5 * torch.randn(*s, device=dev, generator=gen)).requires_grad_(True)
                 for s in ((1, 1, res, res, chn), (1, res, 1, res, chn), (1, res, res, 1, chn))]
        for R in RAYS:
            rays = random_rays(R, gen, dev, mod.rays_encoding_dim)
            leaves = grids + [dec.mlp_params, rays.encoding]
            ups = [torch.randn(R, device=dev, generator=gen), torch.randn(R, device=dev, generator=gen), torch.randn(R, 3, device=dev, generator=gen)]
            plain = lp.Rays(directions=rays.directions, origins=rays.origins, grid_idx=rays.grid_idx, near=rays.near, far=rays.far)
            with torch.no_grad():
                uniform = lp.ray_samples(plain, 128)
                op, _ = lp.lightplane_eval_mlp(uniform.points, grids, rays.grid_idx, dec, rays.encoding, GAIN)
                w = lp.composite_samples(op, None, uniform.depths, uniform.deltas, return_weights=True)[3]
                jitter = torch.rand(R, 128, device=dev, generator=gen)
                fine = lp.importance_samples(plain, uniform.depths, w, 128, jitter=jitter)
                del op, w
            for dname, s in (("S = 128 uniform", uniform), ("S = 256 importance", fine)):
                def chain():
                    opacity, color = lp.lightplane_eval_mlp(s.points, grids, rays.grid_idx, dec, rays.encoding, GAIN)
                    return lp.composite_samples(opacity, color, s.depths, s.deltas)

                def fused():
                    return lp.render_samples(rays, s.depths, s.deltas, grids, dec, gain=GAIN)

                def clear():
                    for t in leaves:
                        t.grad = None

                def forward(fn):
                    with torch.no_grad():
                        return fn()

                def fwd_bwd(fn):
                    clear()
                    torch.autograd.backward(fn(), ups)
                    return [t.grad for t in leaves]

                say(f"\n{sname}, {R} rays, {dname}")
                reps = a.reps * (8 if R <= 4096 else 1)
                for what, run in (("forward", forward), ("forward + backward", fwd_bwd)):
                    r = {"chain": [], "fused": []}
                    for key, fn in (("chain", chain), ("fused", fused)) * 2:
                        r[key].append(timed(lambda: run(fn), reps, a.warmup, clear))
                    for key in ("chain", "fused"):
                        for i, v in enumerate(r[key]):
                            say(f"  {what:18s} {key:6s} pass {i}: {v[0]:9.3f} ms [{v[1]:.3f} .. {v[2]:.3f}]  mem +{v[3] / 2 ** 20:9.1f} MiB")
                    tc, tf = (statistics.median(v[0] for v in r[k]) for k in ("chain", "fused"))
                    spread = abs(r["chain"][0][0] - r["chain"][1][0])
                    mc, mf = (max(v[3] for v in r[k]) for k in ("chain", "fused"))
                    say(f"  {what:18s} chain / fused: time {tc / tf:.2f} x ({tc:.3f} -> {tf:.3f} ms; the chain's two passes differ by "
                        f"{spread:.3f} ms), peak memory {mc / max(mf, 1):.1f} x ({mc / 2 ** 20:.1f} -> {mf / 2 ** 20:.1f} MiB)")
                    x, y = run(chain), run(fused)
                    names = ("ray_length", "neg_log_t", "feature") if what == "forward" else [f"d leaf {i}" for i in range(len(leaves))]
                    say(f"  {what:18s} the two paths differ by at most (of a tensor's max |value|): " + ", ".join(
                        f"{n} {float((p - q).abs().max()) / max(float(p.abs().max()), 1e-30):.1e}" for n, p, q in zip(names, x, y)))
                    tag = f"{sname}, {R} rays, {dname}, {what}"
                    if tf > tc + spread:
                        slower.append(f"{tag}: {tc:.3f} -> {tf:.3f} ms (chain spread {spread:.3f} ms)")
                    if mf >= mc:
                        more_memory.append(f"{tag}: {mc / 2 ** 20:.1f} -> {mf / 2 ** 20:.1f} MiB")
                    clear()
    say("\n# fused slower than the chain by more than the chain's own spread: " + ("nowhere" if not slower else "; ".join(slower)))
    say("# fused peak memory not below the chain's: " + ("nowhere" if not more_memory else "; ".join(more_memory)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

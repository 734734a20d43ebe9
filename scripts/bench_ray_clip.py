#!/usr/bin/env python
"""Developer benchmark of the ray clip (lightplane_amd/ray_clip.py) on one MI355X.

    python scripts/bench_ray_clip.py [--reps 20] [--warmup 3] [--out profiles/ray_clip_bench.txt]

For 65 536 pinhole rays (a 256 x 256 image, camera 2.5 from the centre) and 65 536 random rays (origins on the sphere of radius 2.5, aimed
into the ball of radius 0.8: the recipe of examples/fit_synthetic_scene.py), near 1.2 / far 3.8, against a 128^3 scaffold of a ball of
radius 0.55 with pad = 0.5, it reports
  (a) the clip: as a call -- a device-event window around ONE lp.clip_rays_to_scaffold into preallocated results on an idle queue: the
      wrapper's host time before the launch, the kernel, and the uint8 -> bool kernel behind it -- and as a launch -- 50 lp_rays_clip
      launches through the C ABI back to back between one pair of events, divided by 50: the kernel with its launch gap.  Neither is a
      profiler's kernel time,
  (b) the Renderer's forward + backward at S = 128 on the unclipped rays (LightplaneRenderer 2/2/2 x 32, 128^2 x 16 triplane, the scaffold
      passed, gradients to the planes and the decoder),
  (c) the same on the clipped rays with S' = ceil(128 * mean_span_ratio) samples, i.e. at equal sample density,
and the ratios (b) / (c) and (b) / ((a, call) + (c)).  mean_span_ratio is the mean of (far' - near') / (far - near) over all rays, missed rays (ratio 1) included.
Times are device-event medians over --reps calls after --warmup calls, (b) and (c) alternating in one process, two passes each; min /
max in brackets.  The script needs a GPU and fails without one.
"""
import argparse
import ctypes
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lightplane_amd as lp  # noqa: E402
from lightplane_amd import _lib  # noqa: E402

N_SIDE = 256
S = 128


def timed(fn, reps, warmup):
    """(median ms, min ms, max ms) of fn()"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def pinhole_rays(dev):
    n = N_SIDE * N_SIDE
    u = (torch.arange(N_SIDE, dtype=torch.float32) + 0.5) / N_SIDE * 2.0 - 1.0
    y, x = torch.meshgrid(u, u, indexing="ij")
    d = torch.stack([0.45 * x, 0.45 * y, torch.ones_like(x)], dim=-1).reshape(n, 3)  # the image plane covers +-1.1 at the centre
    d = d / d.norm(dim=-1, keepdim=True)
    rot = torch.tensor([[0.8, 0.0, 0.6], [0.36, 0.8, -0.48], [-0.48, 0.6, 0.64]])  # a rotation: no ray runs along an axis
    d = d @ rot.t()
    o = (-2.5 * rot[:, 2]).expand(n, 3).contiguous()
    return o.to(dev), d.contiguous().to(dev)


def random_rays(dev, gen):
    n = N_SIDE * N_SIDE
    o = torch.randn(n, 3, generator=gen)
    o = 2.5 * o / o.norm(dim=-1, keepdim=True)
    tgt = torch.randn(n, 3, generator=gen)
    tgt = 0.8 * tgt / tgt.norm(dim=-1, keepdim=True) * torch.rand(n, 1, generator=gen) ** (1 / 3)
    d = tgt - o
    return o.to(dev), (d / d.norm(dim=-1, keepdim=True)).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ray_clip.py measures on a GPU; there is nothing to fall back to"
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# ray clip bench  {time.strftime('%Y-%m-%d')}  {torch.cuda.get_device_name(0)}  library src {_lib.build_info()['src_hash'][:16]}")
    say(f"# 65 536 rays, near 1.2 / far 3.8, 128^3 scaffold of a ball of radius 0.55, pad 0.5; Renderer 2/2/2 x 32 on a 128^2 x 16 triplane, "
        f"forward + backward; median of {a.reps} calls after {a.warmup} warm-up calls (device events), min / max in brackets")
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(0)
    c = (torch.arange(128, dtype=torch.float32) + 0.5) / 64.0 - 1.0
    z, y, x = torch.meshgrid(c, c, c, indexing="ij")
    scaffold = ((x * x + y * y + z * z).sqrt() < 0.55).float()[None].contiguous().to(dev)
    say(f"# scaffold occupancy {float(scaffold.mean()):.4f}")
    mod = lp.LightplaneRenderer(num_samples=S, color_chn=3, grid_chn=16, mlp_hidden_chn=32, opacity_init_bias=-2.0, gain=1.0,
                                bg_color=0.0).to(dev)
    shapes = [(1, 1, 128, 128, 16), (1, 128, 1, 128, 16), (1, 128, 128, 1, 16)]
    grids = [torch.nn.Parameter(0.1 * torch.randn(*s, generator=gen).to(dev)) for s in shapes]
    n = N_SIDE * N_SIDE
    for name, (o, d) in (("pinhole", pinhole_rays(dev)), ("random", random_rays(dev, gen))):
        rays = lp.Rays(directions=d, origins=o, grid_idx=torch.zeros(n, dtype=torch.int32, device=dev),
                       near=torch.full((n,), 1.2, device=dev), far=torch.full((n,), 3.8, device=dev), encoding=None)
        out = (torch.empty(n, device=dev), torch.empty(n, device=dev), torch.empty(n, dtype=torch.uint8, device=dev))
        clipped, hit = lp.clip_rays_to_scaffold(rays, scaffold, pad=0.5, out=out)
        ratio = float(((clipped.far - clipped.near) / (rays.far - rays.near)).mean())
        ratio_hit = float(((clipped.far - clipped.near) / (rays.far - rays.near))[hit].mean())
        s_clip = int(math.ceil(S * ratio))
        say(f"\n{name}: hit fraction {float(hit.float().mean()):.3f}, mean span ratio {ratio:.3f} (hit rays alone {ratio_hit:.3f}), S' = {s_clip}")

        def step(r, s):
            for g in grids:
                g.grad = None
            mod.zero_grad(set_to_none=True)
            _, alpha, rgb = mod(r, list(grids), scaffold=scaffold, num_samples=s)
            (rgb.sum() + alpha.sum()).backward()

        ta = timed(lambda: lp.clip_rays_to_scaffold(rays, scaffold, pad=0.5, out=out), 5 * a.reps, a.warmup)
        args = _lib.LpRayClipArgs()
        args.rays = _lib.make_rays(rays.directions, rays.origins, rays.grid_idx, rays.near, rays.far, None)
        args.scaffold, args.scaffold_shape, args.pad = scaffold.data_ptr(), _lib.LpGrid(*scaffold.shape, 0, None), 0.5
        stream, L = _lib.current_stream(dev), _lib.lib()

        def launches():
            for _ in range(50):
                _lib.check(L.lp_rays_clip(ctypes.byref(args), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), stream), "lp_rays_clip")

        tk = tuple(v / 50 for v in timed(launches, a.reps, a.warmup))
        res = {"b": [], "c": []}
        for key in ("b", "c", "b", "c"):
            res[key].append(timed(lambda: step(rays, S) if key == "b" else step(clipped, s_clip), a.reps, a.warmup))
        say(f"  (a) clip, one call of the wrapper        {ta[0]:9.4f} ms [{ta[1]:.4f} .. {ta[2]:.4f}]")
        say(f"  (a) clip, per launch of 50 back to back  {tk[0]:9.4f} ms [{tk[1]:.4f} .. {tk[2]:.4f}]")
        for key, what in (("b", f"(b) render fwd + bwd, unclipped, S = {S}"), ("c", f"(c) render fwd + bwd, clipped, S' = {s_clip}")):
            for i, r in enumerate(res[key]):
                say(f"  {what:40s} pass {i}: {r[0]:9.3f} ms [{r[1]:.3f} .. {r[2]:.3f}]")
        tb = statistics.median(r[0] for r in res["b"])
        tc = statistics.median(r[0] for r in res["c"])
        say(f"  (b) / (c) = {tb / tc:.2f} x;  (a, call) / (b) = {ta[0] / tb:.4f};  (a, launch) / (b) = {tk[0] / tb:.4f};  (b) / ((a, call) + (c)) = {tb / (ta[0] + tc):.2f} x")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

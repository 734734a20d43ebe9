"""Importance resampling (lightplane_amd/importance.py, csrc/lp_importance.hip) against its fp64 definition.

Definition, inputs, the case table and the accuracy bar: tests/importance_cases.py (tests/test_importance_host.py checks them without a
GPU, and shows that the fp32 restatement of the definition meets the bar with a wide margin).  Every new depth of every case is held to
the bar -- F_lower(t (1 - B)) - A <= u_k <= F_upper(t (1 + B)) + A with A = 4 S 2^-24, B = 4 2^-24 -- and the figure is printed before it
is asserted; order and range of the new depths, the merge and the deltas are exact.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

import lightplane_amd as lp
from tests import guarded_alloc as GA
from tests import importance_cases as IC
from tests.test_gpu_parity import _dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worst(name, got, want, tol=IC.TOL):
    """max |err| / max |ref| over every entry, printed and held to the bar"""
    got, want = got.detach().double().cpu(), want.double().cpu()
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    assert bool(torch.isfinite(got).all()), f"{name}: not finite"
    scale = max(float(want.abs().max()), 1e-30)
    err = float((got - want).abs().max()) / scale
    print(f"{name}: max |err| / max |ref| = {err:.3e} (max |ref| {scale:.4g})")
    assert err <= tol, f"{name}: {err:.3e} > {tol}"
    return err


def _rays(c, dev, requires_grad=()):
    t = {k: c[k].to(dev).requires_grad_(k in requires_grad) for k in ("origins", "directions")}
    n = c["origins"].shape[0]
    return lp.Rays(grid_idx=torch.zeros(n, dtype=torch.long, device=dev), near=torch.zeros(n, device=dev), far=torch.ones(n, device=dev), **t)


def _resample(c, dev, N, jitter, include_coarse=True, requires_grad=()):
    rays = _rays(c, dev, requires_grad)
    out = lp.importance_samples(rays, c["depths"].to(dev), c["weights"].to(dev), N, include_coarse=include_coarse, pad=IC.PAD,
                                jitter=c["jitter"].to(dev) if jitter else None)
    return rays, out


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the new depths
# ------------------------------------------------------------------------------------------------------------------------------

def _check_new_depths(name, c, t, N, jitter):
    d = c["depths"]
    R, S = d.shape
    t = t.detach().cpu()
    assert t.shape == (R, N) and bool(torch.isfinite(t).all()), name
    assert bool((t[:, 1:] >= t[:, :-1]).all()), f"{name}: the new depths do not ascend"
    assert bool((t >= d[:, :1]).all()) and bool((t <= d[:, -1:]).all()), f"{name}: a new depth outside [depth_0, depth_(S-1)]"
    jit = c["jitter"] if jitter else None
    ex, _ = IC.bar_excess(t, d, c["weights"], N, IC.PAD, jit)
    print(f"{name}: worst sample {ex:.3f} S 2^-24 outside the B window (the bar: 4)")
    assert ex <= 4.0, f"{name}: {ex:.3f} S 2^-24 > 4"
    return t


@pytest.mark.parametrize("R,S,N", IC.CASES + [IC.LIMIT_CASE])
def test_new_depths_meet_the_bar(R, S, N):
    dev = _dev()
    for regime in IC.REGIMES:
        c = IC.case(R, S, N, regime)
        for jitter in (False, True):
            name = f"R={R} S={S} N={N} {regime}{' jitter' if jitter else ''}"
            _, out = _resample(c, dev, N, jitter, include_coarse=False)
            assert isinstance(out, lp.RaySamples) and out.points.shape == (R, N, 3) and out.deltas.shape == (R, N)
            t = _check_new_depths(name, c, out.depths, N, jitter)
            if regime == "mixed" and R > 1:
                # all-zero rows: the same mass in every bin (tests/importance_cases.py, equal_mass_depths) -- which is uniform in depth,
                # depth_0 + u_k (depth_(S-1) - depth_0), where all bins have one width: S = 2
                jz = c["jitter"][1::3] if jitter else None
                _worst(f"{name} all-zero rows vs equal mass per bin", t[1::3], IC.equal_mass_depths(c["depths"][1::3], N, jz), tol=1e-6)
                if S == 2:
                    dz = c["depths"][1::3].double()
                    uniform = dz[:, :1] + IC.targets(dz.shape[0], N, jz, torch.float64) * (dz[:, -1:] - dz[:, :1])
                    _worst(f"{name} all-zero rows vs uniform in depth", t[1::3], uniform, tol=1e-6)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. merge, deltas, points
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R,S,N", IC.CASES + [IC.LIMIT_CASE])
def test_merge_deltas_and_points(R, S, N):
    dev = _dev()
    for regime in IC.REGIMES:
        c = IC.case(R, S, N, regime)
        for jitter in (False, True):
            name = f"R={R} S={S} N={N} {regime}{' jitter' if jitter else ''}"
            _, alone = _resample(c, dev, N, jitter, include_coarse=False)
            _, out = _resample(c, dev, N, jitter)
            assert out.points.shape == (R, S + N, 3) and out.depths.shape == out.deltas.shape == (R, S + N)
            t = alone.depths
            want = torch.sort(torch.cat([c["depths"].to(dev), t], dim=1), dim=1).values
            assert torch.equal(out.depths, want), f"{name}: depths' is not the sorted union of the coarse depths and the kernel's own t"
            for label, o in (("merged", out), ("alone", alone)):
                d = o.depths
                diff = d[:, 1:] - d[:, :-1]
                first = diff[:, :1] if d.shape[1] > 1 else torch.ones_like(d)
                assert torch.equal(o.deltas, torch.cat([first, diff], dim=1)), f"{name} {label}: deltas' are not the fp32 differences"
                f32 = IC.assemble(c["origins"], c["directions"], c["depths"], d.cpu(), False, torch.float32)[0]
                f64 = IC.assemble(c["origins"], c["directions"], c["depths"], d.cpu(), False, torch.float64)[0]
                _worst(f"{name} {label} points vs the fp32 formula", o.points, f32, tol=1e-6)
                _worst(f"{name} {label} points vs fp64", o.points, f64)
            # and the whole result against the fp64 definition's own merge of the kernel's t: deltas included
            ref = IC.assemble(c["origins"], c["directions"], c["depths"], t.cpu(), True, torch.float64)
            assert torch.equal(out.depths.cpu().double(), ref[1])


# ------------------------------------------------------------------------------------------------------------------------------
# 3. backward
# ------------------------------------------------------------------------------------------------------------------------------

def _backward(c, dev, N, requires_grad, include_coarse=True):
    rays, out = _resample(c, dev, N, True, include_coarse, requires_grad)
    g = c["g_points"].to(dev) if include_coarse else c["g_points"][:, :N].to(dev)
    (out.points * g).sum().backward()
    return rays, out


@pytest.mark.parametrize("R,S,N", [(1, 2, 1), (63, 3, 2), (130, 63, 65), (63, 64, 64), (130, 65, 63), (63, 131, 130), IC.LIMIT_CASE])
def test_backward(R, S, N):
    dev = _dev()
    c = IC.case(R, S, N, "mixed")
    for include_coarse in (True, False):
        name = f"R={R} S={S} N={N}{'' if include_coarse else ' alone'}"
        w = c["weights"].to(dev).requires_grad_(True)
        d = c["depths"].to(dev).requires_grad_(True)
        rays = _rays(c, dev, ("origins", "directions"))
        out = lp.importance_samples(rays, d, w, N, include_coarse=include_coarse, jitter=c["jitter"].to(dev))
        assert out.points.requires_grad and out.depths.requires_grad is False and out.deltas.requires_grad is False
        g = c["g_points"] if include_coarse else c["g_points"][:, :N]
        (out.points * g.to(dev)).sum().backward()
        assert w.grad is None and d.grad is None
        leaves = {k: c[k].double().requires_grad_(True) for k in ("origins", "directions")}
        ref = out.depths.detach().cpu().double()[..., None] * leaves["directions"][:, None] + leaves["origins"][:, None]
        (ref * g.double()).sum().backward()
        full = {}
        for k, leaf in leaves.items():
            full[k] = getattr(rays, k).grad
            _worst(f"{name} d {k}", full[k], leaf.grad)
        for only in ("origins", "directions"):
            r1, _ = _backward(c, dev, N, (only,), include_coarse)
            other = "directions" if only == "origins" else "origins"
            assert getattr(r1, other).grad is None
            assert torch.equal(getattr(r1, only).grad, full[only]), f"{name}: d {only} alone differs from the full run"
    # no gradient asked for / nothing upstream of the points: nothing runs, nothing fails
    rays, out = _resample(c, dev, N, True, True, ("origins",))
    assert out.depths.requires_grad is False
    rays, out = _resample(c, dev, N, True)
    assert not out.points.requires_grad


# ------------------------------------------------------------------------------------------------------------------------------
# 4. hygiene
# ------------------------------------------------------------------------------------------------------------------------------

def test_two_runs_are_bit_identical():
    dev = _dev()
    for key in ((130, 131, 130, "transparent"), (63, 65, 63, "mixed"), (130, 64, 65, "duplicates")):
        c = IC.case(*key)
        runs = []
        for _ in range(2):
            rays, out = _backward(c, dev, key[2], ("origins", "directions"))
            runs.append(tuple(out) + (rays.origins.grad, rays.directions.grad))
        assert all(torch.equal(a, b) for a, b in zip(*runs)), key


@pytest.mark.parametrize("pattern", GA.PATTERNS)
def test_every_buffer_is_written_entirely(pattern):
    """forward and backward under poisoned, fenced allocations: no element of a result or a gradient keeps the poison and every fence is
    intact (checked when the block ends)"""
    dev = _dev()
    with GA.guarded(pattern) as g:
        for key in ((63, 65, 63, "mixed"), (130, 131, 2, "transparent"), (1, 2, 1, "opaque"), (63, 3, 130, "duplicates"), (3, 2048, 2048, "mixed")):
            c = IC.case(*key)
            for include_coarse in (True, False):
                _backward(c, dev, key[2], ("origins", "directions"), include_coarse)
                _backward(c, dev, key[2], ("directions",), include_coarse)
                _resample(c, dev, key[2], False, include_coarse)
        torch.cuda.synchronize()
        records = g.from_file("lightplane_amd/importance.py")
        poisoned = [r for r in records if r.poisoned]
        assert len(poisoned) >= 5 * 2 * (3 * 3 + 3), len(poisoned)
        for r in poisoned:
            assert g.unwritten(r) == 0, f"{g.unwritten(r)} of {r.payload.numel()} elements unwritten: {r.where()}"


def test_empty_batch():
    dev = _dev()
    z = lambda *s: torch.zeros(*s, device=dev, requires_grad=True)  # noqa: E731
    rays = lp.Rays(directions=z(0, 3), origins=z(0, 3), grid_idx=torch.zeros(0, dtype=torch.long, device=dev), near=z(0), far=z(0))
    out = lp.importance_samples(rays, torch.zeros(0, 5, device=dev), torch.zeros(0, 5, device=dev), 7)
    assert out.points.shape == (0, 12, 3) and out.depths.shape == out.deltas.shape == (0, 12)
    out.points.sum().backward()
    assert rays.origins.grad.shape == (0, 3) and rays.directions.grad.shape == (0, 3)
    out = lp.importance_samples(rays, torch.zeros(0, 5, device=dev), torch.zeros(0, 5, device=dev), 7, include_coarse=False,
                                jitter=torch.zeros(0, 7, device=dev))
    assert out.points.shape == (0, 7, 3)
    torch.cuda.synchronize()


def test_memory_is_the_results():
    """a no-grad call allocates its results and (allocator rounding aside) nothing else: the bound of
    tests/test_gpu_compositing.py::test_memory_is_the_results"""
    dev = _dev()
    R, S, N = 2048, 128, 128
    c = IC.inputs(R, S, N, "transparent")
    rays = _rays(c, dev)
    depths, weights, jitter = (c[k].to(dev) for k in ("depths", "weights", "jitter"))
    with torch.no_grad():
        lp.importance_samples(rays, depths, weights, N, jitter=jitter)  # (library and kernel are loaded)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        out = lp.importance_samples(rays, depths, weights, N, jitter=jitter)
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated(dev) - before
        results = 4 * R * (S + N) * 5
        print(f"importance_samples: peak extra memory {extra} bytes for results of {results}")
        assert extra <= 1.25 * results + 64 * 1024, f"{extra} bytes beyond the inputs for {results} bytes of results"
        del out


def _warm_up(fn, times=1):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(times):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


def test_graph_capture_with_replay_on_new_weights():
    """forward + backward captured once on one stream and replayed on new weights: every replay equals the eager run on the same
    values to the bit"""
    dev = _dev()
    c = IC.case(130, 65, 63, "transparent")
    rays = _rays(c, dev, ("origins", "directions"))
    depths, weights, jitter, g = (c[k].to(dev) for k in ("depths", "weights", "jitter", "g_points"))
    weights = weights.clone()

    def step():
        rays.origins.grad = rays.directions.grad = None
        out = lp.importance_samples(rays, depths, weights, 63, jitter=jitter)
        (out.points * g).sum().backward()
        return out

    _warm_up(step, 3)
    rays.origins.grad = rays.directions.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    captured = [rays.origins.grad, rays.directions.grad]
    first = None
    for round_ in range(2):
        if round_ == 1:  # new values in the tensor the graph reads
            with torch.no_grad():
                weights.copy_(IC.case(130, 65, 63, "opaque")["weights"].to(dev))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.detach().clone() for t in tuple(out) + tuple(captured)]
        eager = step()
        for i, (a, b) in enumerate(zip(replayed, tuple(eager) + (rays.origins.grad, rays.directions.grad))):
            assert torch.equal(a, b.detach()), f"round {round_}: replayed tensor {i} != eager"
        if round_ == 0:
            first = replayed[1].clone()
    assert float((replayed[1] - first).abs().max()) > 1e-4  # (the second round really saw other weights)


def test_module_glue_is_the_function():
    dev = _dev()
    mod = lp.LightplaneRenderer(num_samples=17, color_chn=3, grid_chn=16, mlp_hidden_chn=32).to(dev)
    c = IC.case(63, 65, 63, "mixed")
    rays = _rays(c, dev)
    samples = lp.RaySamples(None, c["depths"].to(dev), None)
    w, jit = c["weights"].to(dev), c["jitter"].to(dev)
    for kw in ({}, dict(include_coarse=False, pad=1e-3, jitter=jit)):
        a, b = mod.importance_samples(rays, samples, w, 63, **kw), lp.importance_samples(rays, samples.depths, w, 63, **kw)
        assert isinstance(a, lp.RaySamples) and all(torch.equal(x, y) for x, y in zip(a, b))
    assert a.depths.shape == (63, 63)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. the chain, the example
# ------------------------------------------------------------------------------------------------------------------------------

def test_the_coarse_to_fine_chain_runs_with_gradients_to_the_origins():
    """ray_samples(S = 32) -> analytic density -> composite_samples(return_weights) -> importance_samples(N = 32) -> the density again
    -> composite_samples, against the same chain in fp64 on the kernel's own fine depths"""
    dev = _dev()
    R = 130
    gen = torch.Generator().manual_seed(5)
    origins = torch.tensor([0.0, 0.0, -2.5]) + 0.05 * torch.randn(R, 3, generator=gen)
    directions = torch.nn.functional.normalize(torch.tensor([0.0, 0.0, 1.0]) + 0.08 * torch.randn(R, 3, generator=gen), dim=-1)
    o = origins.to(dev).requires_grad_(True)
    rays = lp.Rays(directions=directions.to(dev), origins=o, grid_idx=torch.zeros(R, dtype=torch.long, device=dev),
                   near=torch.full((R,), 1.0, device=dev), far=torch.full((R,), 4.0, device=dev))

    def density(p):  # a soft ball of radius 0.5
        return 20.0 * torch.sigmoid(40.0 * (0.5 - p.norm(dim=-1)))

    def color(p):
        return torch.sigmoid(3.0 * p)

    with torch.no_grad():
        coarse = lp.ray_samples(rays, 32)
        _, _, _, w = lp.composite_samples(density(coarse.points), color(coarse.points), coarse.depths, coarse.deltas, return_weights=True)
    fine = lp.importance_samples(rays, coarse.depths, w, 32)
    assert fine.points.shape == (R, 64, 3) and fine.points.requires_grad and not fine.depths.requires_grad
    length, nlt, rgb = lp.composite_samples(density(fine.points), color(fine.points), fine.depths, fine.deltas)
    (length.sum() + nlt.sum() + rgb.sum()).backward()
    assert o.grad is not None and bool(torch.isfinite(o.grad).all()) and float(o.grad.abs().max()) > 0
    # the fine samples crowd where the coarse weights are: more than half of the new depths within the ball's shell of depth
    hit = w.sum(-1) > 0.5
    assert int(hit.sum()) > R // 2
    spread_fine = (fine.depths[hit].std(-1)).mean()
    assert float(spread_fine) < float(coarse.depths[hit].std(-1).mean())
    # the same chain in fp64 at the kernel's fine depths
    o64 = origins.double().requires_grad_(True)
    d64, dl64 = fine.depths.detach().cpu().double(), fine.deltas.detach().cpu().double()
    p64 = d64[..., None] * directions.double()[:, None] + o64[:, None]
    od = density(p64) * dl64
    T = torch.exp(-torch.cumsum(torch.nn.functional.pad(od, (1, 0)), -1))
    w64 = T[:, :-1] - T[:, 1:]
    ref = ((w64 * d64).sum(-1), od.sum(-1), (w64[..., None] * color(p64)).sum(-2))
    for key, a, b in zip(("ray_length", "neg_log_t", "feature"), (length, nlt, rgb), ref):
        _worst(f"coarse -> fine {key}", a, b.detach())
    (ref[0].sum() + ref[1].sum() + ref[2].sum()).backward()
    _worst("coarse -> fine d origins", o.grad, o64.grad)


def test_example_fits_through_the_coarse_to_fine_march():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "fit_synthetic_scene.py"), "--modular", "--importance", "32", "--steps", "20",
                        "--rays", "2048"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = r.stdout.decode()
    assert r.returncode == 0, text
    out = json.loads(text.strip().splitlines()[-1])
    print(out)
    assert out["modular"] is True and out["importance"] == 32 and out["steps"] == 20 and out["last_loss"] < out["first_loss"], out

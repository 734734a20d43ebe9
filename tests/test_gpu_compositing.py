"""The modular march (lightplane_amd/compositing.py, csrc/lp_composite.hip) against its fp64 definitions.

Definitions, inputs and the case table: tests/compositing_cases.py (tests/test_compositing_host.py checks them without a GPU).  Every
comparison is held to the project's bar, max |err| / max |ref| <= 1e-4 per tensor, and prints its figure before it asserts; no entry
of a compositing result or gradient is left out.  The sample placement is also held to the oracle's fp32 formulas at 1e-6 of max
(eight fp32 ulps: a fused against an unfused multiply-add differs by one ulp per operation).
"""
import itertools
import json
import os
import subprocess
import sys

import pytest
import torch

import lightplane_amd as lp
from tests import compositing_cases as CC
from tests import guarded_alloc as GA
from tests.synth import random_rays
from tests.test_gpu_parity import _dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUT_KEYS = ("opacity", "features", "depths", "deltas")


def _worst(name, got, want, tol=CC.TOL):
    """max |err| / max |ref| over every entry, printed and held to the bar"""
    got, want = got.detach().double().cpu(), want.double().cpu()
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    assert bool(torch.isfinite(got).all()), f"{name}: not finite"
    if want.numel() == 0:
        return 0.0
    scale = max(float(want.abs().max()), 1e-30)
    err = float((got - want).abs().max()) / scale
    print(f"{name}: max |err| / max |ref| = {err:.3e} (max |ref| {scale:.4g})")
    assert err <= tol, f"{name}: {err:.3e} > {tol}"
    return err


# ------------------------------------------------------------------------------------------------------------------------------
# 1. placement
# ------------------------------------------------------------------------------------------------------------------------------

def _rays(R, dev, seed, requires_grad=False):
    r = random_rays(torch.Generator().manual_seed(seed), R, 2, None)
    t = {k: getattr(r, k).to(dev) for k in ("directions", "origins", "near", "far")}
    if requires_grad:
        for v in t.values():
            v.requires_grad_(True)
    return r, lp.Rays(grid_idx=r.grid_idx.to(dev), encoding=None, **t)


@pytest.mark.parametrize("S_inf", [0, 3])
@pytest.mark.parametrize("S", [1, 2, 63, 64, 65])
def test_placement(S, S_inf):
    dev = _dev()
    for R in (1, 63, 130):
        name = f"R={R} S={S} S_inf={S_inf}"
        cpu, rays = _rays(R, dev, 100 * S + 10 * S_inf + R, requires_grad=True)
        got = lp.ray_samples(rays, S, S_inf, disparity_at_inf=1e-5)
        assert isinstance(got, lp.RaySamples) and got.points.shape == (R, S + S_inf, 3) and got.depths.shape == got.deltas.shape == (R, S + S_inf)
        f32 = CC.placement(cpu, S, S_inf, 1e-5, torch.float32)
        f64 = CC.placement(cpu, S, S_inf, 1e-5, torch.float64)
        for key, g, a, b in zip(("points", "depths", "deltas"), got, f32, f64):
            _worst(f"{name} {key} vs the fp32 formulas", g, a, tol=1e-6)
            _worst(f"{name} {key} vs fp64", g, b)
        # gradients with a random upstream on all three results
        gen = torch.Generator().manual_seed(7 + S)
        ups = [torch.randn(t.shape, generator=gen) for t in got]
        sum((g * u.to(dev)).sum() for g, u in zip(got, ups)).backward()
        leaves = {k: getattr(cpu, k).double().requires_grad_(True) for k in ("origins", "directions", "near", "far")}
        ref = CC.placement(lp.Rays(grid_idx=cpu.grid_idx, **leaves), S, S_inf, 1e-5, torch.float64)
        sum((g * u.double()).sum() for g, u in zip(ref, ups)).backward()
        for k, leaf in leaves.items():
            _worst(f"{name} d {k}", getattr(rays, k).grad, leaf.grad)


def test_placement_is_the_module_s():
    dev = _dev()
    mod = lp.LightplaneRenderer(num_samples=17, color_chn=3, grid_chn=16, mlp_hidden_chn=32, num_samples_inf=2, disparity_at_inf=1e-3).to(dev)
    _, rays = _rays(5, dev, 3)
    a, b = mod.ray_samples(rays), lp.ray_samples(rays, 17, 2, disparity_at_inf=1e-3)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and a.depths.shape == (5, 19)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. compositing: values and gradients
# ------------------------------------------------------------------------------------------------------------------------------

def _leaves(c, dev, requires_grad=INPUT_KEYS):
    return [None if c[k] is None else c[k].to(dev).requires_grad_(k in requires_grad) for k in INPUT_KEYS]


def _run(c, dev, return_weights, requires_grad=INPUT_KEYS, upstream=("g_len", "g_nlt", "g_feat", "g_w")):
    """forward and backward of one case: (results, gradients); an upstream gradient only on the results named"""
    leaves = _leaves(c, dev, requires_grad)
    out = lp.composite_samples(*leaves, return_weights=return_weights)
    loss = 0.0
    for o, key in zip(out, ("g_len", "g_nlt", "g_feat", "g_w")):
        if o is not None and key in upstream:
            loss = loss + (o * c[key].to(dev)).sum()
    if torch.is_tensor(loss) and loss.requires_grad:
        loss.backward()
    return out, [None if t is None else t.grad for t in leaves]


@pytest.mark.parametrize("regime", CC.REGIMES)
@pytest.mark.parametrize("R,S,C", CC.CASES)
def test_values_and_gradients(R, S, C, regime):
    dev, c = _dev(), CC.case(R, S, C, regime)
    for return_weights in (False, True):
        name = f"R={R} S={S} C={C} {regime}{' +weights' if return_weights else ''}"
        out, grads = _run(c, dev, return_weights)
        assert len(out) == (4 if return_weights else 3) and (out[2] is None) == (C == 0)
        for key, o, want in zip(("ray_length", "neg_log_t", "feature", "weights"), out, c["out"]):
            if o is not None:
                _worst(f"{name} {key}", o, want)
        for key, g, want in zip(INPUT_KEYS, grads, c["grads_w" if return_weights else "grads"]):
            if want is not None:
                _worst(f"{name} d {key}", g, want)


@pytest.mark.parametrize("regime", ["transparent", "mixed"])
def test_a_ray_longer_than_the_backward_s_carry_table(regime):
    """33 000 samples are 516 chunks of 64: the backward keeps the -log T of 512 chunk starts in LDS at a time and does such a ray in
    two super-blocks from the far end (csrc/lp_composite.hip, CB_SUPER) -- the one size at which it takes another path"""
    dev, c = _dev(), CC.case(2, 33000, 3, regime)
    out, grads = _run(c, dev, True)
    for key, o, want in zip(("ray_length", "neg_log_t", "feature", "weights"), out, c["out"]):
        _worst(f"S=33000 {regime} {key}", o, want)
    for key, g, want in zip(INPUT_KEYS, grads, c["grads_w"]):
        _worst(f"S=33000 {regime} d {key}", g, want)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. partial gradients, 4. bit-reproducibility
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [5, 32, 67])  # (one float per lane, four floats per lane, two units per lane: the three instantiations)
def test_partial_gradients_are_the_full_ones_bit_for_bit(C):
    dev, c = _dev(), CC.case(63, 131, C, "mixed")
    for up in ("g_len", "g_nlt", "g_feat", "g_w"):
        _, full = _run(c, dev, True, upstream=(up,))
        assert all(g is not None and bool(torch.isfinite(g).all()) for g in full)
        for n in range(5):
            for subset in itertools.combinations(INPUT_KEYS, n):
                _, grads = _run(c, dev, True, requires_grad=subset, upstream=(up,))
                for key, g, f in zip(INPUT_KEYS, grads, full):
                    if key in subset:
                        assert g is not None and torch.equal(g, f), f"upstream {up}, requires_grad {subset}: d {key} differs from the full run"
                    else:
                        assert g is None, f"upstream {up}, requires_grad {subset}: {key} got a gradient"


def test_two_runs_are_bit_identical():
    dev = _dev()
    for key in ((130, 200, 128, "transparent"), (63, 65, 3, "mixed"), (130, 131, 67, "opaque")):
        c = CC.case(*key)
        (o1, g1), (o2, g2) = _run(c, dev, True), _run(c, dev, True)
        assert all(torch.equal(a, b) for a, b in zip(o1 + tuple(g1), o2 + tuple(g2))), key
    _, rays = _rays(130, dev, 9, requires_grad=True)
    runs = []
    for _ in range(2):
        for t in (rays.origins, rays.directions, rays.near, rays.far):
            t.grad = None
        s = lp.ray_samples(rays, 65, 3)
        (s.points.sum() + (s.depths * s.deltas).sum()).backward()
        runs.append(tuple(s) + tuple(t.grad.clone() for t in (rays.origins, rays.directions, rays.near, rays.far)))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


# ------------------------------------------------------------------------------------------------------------------------------
# 5. unwritten buffers
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", GA.PATTERNS)
def test_every_buffer_is_written_entirely(pattern):
    """forward and backward of both ops under poisoned, fenced allocations: no element of a result or a gradient keeps the poison and
    every fence is intact (checked when the block ends)"""
    dev = _dev()
    with GA.guarded(pattern) as g:
        for key in ((63, 65, 5, "mixed"), (130, 131, 32, "transparent"), (1, 200, 67, "opaque"), (63, 2, 0, "mixed")):
            _run(CC.case(*key), dev, True)
            _run(CC.case(*key), dev, False, upstream=())  # (no upstream gradient: nothing runs backward)
        for S, S_inf in ((65, 3), (1, 0)):
            _, rays = _rays(63, dev, 5, requires_grad=True)
            s = lp.ray_samples(rays, S, S_inf)
            (s.points.sum() + s.depths.sum() + s.deltas.sum()).backward()
            _, rays = _rays(63, dev, 5, requires_grad=True)
            lp.ray_samples(rays, S, S_inf).depths.sum().backward()  # (upstream on one result only)
        torch.cuda.synchronize()
        records = g.from_file("lightplane_amd/compositing.py")
        poisoned = [r for r in records if r.poisoned]
        assert len(poisoned) >= 40, len(poisoned)
        for r in poisoned:
            assert g.unwritten(r) == 0, f"{g.unwritten(r)} of {r.payload.numel()} elements unwritten: {r.where()}"


# ------------------------------------------------------------------------------------------------------------------------------
# 6. empty batch, allocator state
# ------------------------------------------------------------------------------------------------------------------------------

def test_empty_batch():
    dev = _dev()
    z = lambda *s: torch.zeros(*s, device=dev, requires_grad=True)  # noqa: E731
    rays = lp.Rays(directions=z(0, 3), origins=z(0, 3), grid_idx=torch.zeros(0, dtype=torch.long, device=dev), near=z(0), far=z(0))
    s = lp.ray_samples(rays, 5, 2)
    assert s.points.shape == (0, 7, 3) and s.depths.shape == s.deltas.shape == (0, 7)
    (s.points.sum() + s.deltas.sum()).backward()
    assert rays.origins.grad.shape == (0, 3) and rays.far.grad.shape == (0,)
    o, f, d, dl = z(0, 7), z(0, 7, 4), z(0, 7), z(0, 7)
    length, nlt, feat, w = lp.composite_samples(o, f, d, dl, return_weights=True)
    assert length.shape == nlt.shape == (0,) and feat.shape == (0, 4) and w.shape == (0, 7)
    (length.sum() + feat.sum() + w.sum()).backward()
    assert o.grad.shape == (0, 7) and f.grad.shape == (0, 7, 4)
    length, nlt, feat = lp.composite_samples(o.detach(), None, d.detach(), dl.detach())
    assert feat is None and length.shape == (0,)
    torch.cuda.synchronize()


def test_memory_is_the_results():
    """a no-grad call allocates its results and (allocator rounding aside) nothing else: the bound of
    tests/test_gpu_points.py::test_memory_is_the_two_results"""
    dev = _dev()
    R, S, C = 2048, 128, 32
    gen = torch.Generator().manual_seed(5)
    _, rays = _rays(R, dev, 11)
    opacity, deltas = torch.rand(R, S, generator=gen).to(dev), (torch.rand(R, S, generator=gen) * 0.05).to(dev)
    depths, features = torch.rand(R, S, generator=gen).to(dev), torch.randn(R, S, C, generator=gen).to(dev)
    with torch.no_grad():
        lp.ray_samples(rays, 2)
        lp.composite_samples(opacity[:1], features[:1], depths[:1], deltas[:1], return_weights=True)  # (library and kernels are loaded)
        for what, fn, results in (("ray_samples", lambda: lp.ray_samples(rays, S - 3, 3), 4 * R * S * 5),
                                  ("composite_samples", lambda: lp.composite_samples(opacity, features, depths, deltas, return_weights=True),
                                   4 * R * (2 + C + S))):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            before = torch.cuda.memory_allocated(dev)
            out = fn()
            torch.cuda.synchronize()
            extra = torch.cuda.max_memory_allocated(dev) - before
            print(f"{what}: peak extra memory {extra} bytes for results of {results}")
            assert extra <= 1.25 * results + 64 * 1024, f"{what}: {extra} bytes beyond the inputs for {results} bytes of results"
            del out


# ------------------------------------------------------------------------------------------------------------------------------
# 7. graph capture
# ------------------------------------------------------------------------------------------------------------------------------

def _warm_up(fn, times=1):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(times):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


def test_graph_capture_forward_and_backward():
    """ray_samples -> (a decoder of the test's own, in PyTorch) -> composite_samples, forward + backward captured once on one stream and
    replayed on new ray values: every replay equals the eager run on the same values to the bit (no atomics anywhere in the chain's
    own kernels, and the PyTorch ops in between are elementwise)"""
    dev = _dev()
    _, rays = _rays(130, dev, 21, requires_grad=True)
    leaves = [rays.origins, rays.directions, rays.near, rays.far]
    gen = torch.Generator().manual_seed(3)
    ups = [torch.randn(130, generator=gen).to(dev), torch.randn(130, generator=gen).to(dev), torch.randn(130, 3, generator=gen).to(dev),
           torch.randn(130, 68, generator=gen).to(dev)]

    def step():
        for t in leaves:
            t.grad = None
        s = lp.ray_samples(rays, 65, 3)
        opacity = torch.exp(-4.0 * (s.points * s.points).sum(-1))  # a soft ball
        color = torch.sigmoid(3.0 * s.points)
        out = lp.composite_samples(opacity, color, s.depths, s.deltas, return_weights=True)
        sum((o * u).sum() for o, u in zip(out, ups)).backward()
        return out

    _warm_up(step, 3)
    for t in leaves:
        t.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    captured = [t.grad for t in leaves]
    gen = torch.Generator().manual_seed(77)
    first = None
    for round_ in range(2):
        if round_ == 1:  # new values in the tensors the graph reads
            with torch.no_grad():
                rays.origins.add_(0.05 * torch.randn(130, 3, generator=gen).to(dev))
                rays.far.mul_(0.9)
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.detach().clone() for t in tuple(out) + tuple(captured)]
        eager = step()
        for i, (a, b) in enumerate(zip(replayed, tuple(eager) + tuple(t.grad for t in leaves))):
            assert torch.equal(a, b.detach()), f"round {round_}: replayed tensor {i} != eager"
        if round_ == 0:
            first = replayed[0].clone()
    assert float((replayed[0] - first).abs().max()) > 1e-4  # (the second round really saw other rays)


# ------------------------------------------------------------------------------------------------------------------------------
# 8. the chain is the Renderer
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CC.CHAIN_CASES))
def test_the_chain_is_the_renderer(name):
    from tests import points_cases as PC
    dev, c = _dev(), CC.chain_case(name)
    assert int(c["kink"].sum()) <= PC.MAX_LEFT_OUT * c["kink"].numel()
    r = c["rays"]
    t = {k: getattr(r, k).to(dev).requires_grad_(True) for k in ("origins", "directions", "near", "far")}
    rays = lp.Rays(grid_idx=r.grid_idx.to(dev), encoding=r.encoding.to(dev), **t)
    grids = [g.to(dev).requires_grad_(True) for g in c["grids"]]
    dec = lp.DecoderParams(c["dec"].mlp_params.to(dev).requires_grad_(True), c["dec"].n_hidden_trunk, c["dec"].n_hidden_opacity, c["dec"].n_hidden_color, 3)
    s = lp.ray_samples(rays, CC.CHAIN_S, CC.CHAIN_S_INF, disparity_at_inf=CC.CHAIN_DISPARITY)
    live = torch.where(c["kink"].to(dev)[..., None], s.points.detach(), s.points)  # (tests/compositing_cases.py: chain_case)
    opacity, color = lp.lightplane_eval_mlp(live, grids, rays.grid_idx, dec, rays.encoding, CC.CHAIN_GAIN, contract_coords=c["contract"])
    out = lp.composite_samples(opacity, color, s.depths, s.deltas)
    with torch.no_grad():
        fused = lp.lightplane_renderer(rays, grids, dec, num_samples=CC.CHAIN_S, gain=CC.CHAIN_GAIN, num_samples_inf=CC.CHAIN_S_INF,
                                       contract_coords=c["contract"], disparity_at_inf=CC.CHAIN_DISPARITY)
    for key, o, want, f in zip(("ray_length", "neg_log_t", "feature"), out, c["out"], fused):
        _worst(f"{name} {key} vs the fp64 oracle Renderer", o, want)
        _worst(f"{name} {key} vs the fused Renderer on the GPU", o, f, tol=2e-4)
    sum((o * u.to(dev)).sum() for o, u in zip(out, c["ups"])).backward()
    for k, leaf in t.items():
        _worst(f"{name} d {k}", leaf.grad, c["grads"][k])
    for i, (g, want) in enumerate(zip(grids, c["grads"]["grids"])):
        _worst(f"{name} d grid[{i}]", g.grad, want)
    _worst(f"{name} d mlp_params", dec.mlp_params.grad, c["grads"]["mlp_params"])


# ------------------------------------------------------------------------------------------------------------------------------
# 9. example
# ------------------------------------------------------------------------------------------------------------------------------

def test_example_fits_through_the_modular_march():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "fit_synthetic_scene.py"), "--modular", "--steps", "20", "--rays", "2048"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = r.stdout.decode()
    assert r.returncode == 0, text
    out = json.loads(text.strip().splitlines()[-1])
    print(out)
    assert out["modular"] is True and out["steps"] == 20 and out["last_loss"] < out["first_loss"], out

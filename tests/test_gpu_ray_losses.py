"""The distortion loss and the interlevel loss (lightplane_amd/ray_losses.py, csrc/lp_ray_losses.hip) against their fp64 definitions.

Definitions, inputs, the case tables and the bars: tests/ray_loss_cases.py (tests/test_ray_losses_host.py checks them without a GPU and
shows that the fp32 restatement of the forms the kernels use meets the bars).  Every result and gradient is held to 1e-4 of its
tensor's max; where the weights and deltas are non-negative every ray's distortion loss and every entry of its gradient to the weights
is additionally held to 4 S 2^-24 relative.  Every figure is printed before it is asserted.

Worst figures measured on an MI355X: distortion loss 1.3e-7, d weights 2.6e-7, d depths 3.2e-7, d deltas 7.1e-8 of max;
entry-wise 1.18 S 2^-24 (loss) and 1.13 S 2^-24 (d weights), both at S = 1; interlevel loss 5.4e-8, d proposal_weights 5.0e-8 of max.
"""
import ctypes
import itertools
import json
import os
import subprocess
import sys

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib
from tests import guarded_alloc as GA
from tests import ray_loss_cases as LC
from tests.test_gpu_parity import _dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIST_KEYS = ("weights", "depths", "deltas")
INTER_KEYS = ("weights", "depths", "proposal_weights", "proposal_depths")


def _worst(name, got, want, tol=LC.TOL):
    """max |err| / max |ref| over every entry, printed and held to the bar"""
    got, want = got.detach().double().cpu(), want.double().cpu()
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    assert bool(torch.isfinite(got).all()), f"{name}: not finite"
    scale = max(float(want.abs().max()), 1e-30)
    err = float((got - want).abs().max()) / scale
    print(f"{name}: max |err| / max |ref| = {err:.3e} (max |ref| {scale:.4g})")
    assert err <= tol, f"{name}: {err:.3e} > {tol}"
    return err


def _entrywise(name, got, want, S):
    """every entry against its own reference: |err| <= 4 S 2^-24 |ref| (sums of non-negative terms)"""
    got, want = got.detach().double().cpu(), want.double().cpu()
    err = (got - want).abs()
    worst = float((err / want.abs().clamp(min=1e-300)).max()) / (S * LC.EPS24)
    print(f"{name}: worst entry {worst:.3f} S 2^-24 relative (the bar: 4)")
    assert bool((err <= LC.bar_sum(S) * want.abs()).all()), f"{name}: {worst:.3f} S 2^-24 > 4"


def _distortion(c, dev, requires_grad=DIST_KEYS, g=None):
    t = {k: c[k].to(dev).requires_grad_(k in requires_grad) for k in DIST_KEYS}
    loss = lp.distortion_loss(t["weights"], t["depths"], t["deltas"])
    if requires_grad:
        (loss.sum() if g is None else (loss * g.to(dev)).sum()).backward()
    return loss, t


def _interlevel(c, dev, requires_grad=True, g=None, eps=LC.EPS):
    t = {k: c[k].to(dev) for k in INTER_KEYS}
    t["proposal_weights"].requires_grad_(requires_grad)
    loss = lp.interlevel_loss(t["weights"], t["depths"], t["proposal_weights"], t["proposal_depths"], eps=eps)
    if requires_grad:
        (loss.sum() if g is None else (loss * g.to(dev)).sum()).backward()
    return loss, t


# ------------------------------------------------------------------------------------------------------------------------------
# 1. values and gradients
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R,S", LC.DIST_CASES + [LC.DIST_LIMIT])
def test_distortion_values_and_gradients(R, S):
    dev = _dev()
    for regime in LC.DIST_REGIMES:
        c = LC.distortion_case(R, S, regime)
        name = f"distortion R={R} S={S} {regime}"
        loss, t = _distortion(c, dev)
        assert loss.shape == (R,) and loss.dtype == torch.float32
        ref = c["ref"]
        _worst(f"{name} loss", loss, ref[0])
        for k, want in zip(DIST_KEYS, ref[1:]):
            _worst(f"{name} d {k}", t[k].grad, want)
        if regime in LC.NONNEG:
            _entrywise(f"{name} loss", loss, ref[0], S)
            _entrywise(f"{name} d weights", t["weights"].grad, ref[1], S)
        if regime == "mixed" and R > 1:  # all-zero rows: no loss, no gradient, exactly
            assert float(loss[1::3].abs().max()) == 0.0 and all(float(t[k].grad[1::3].abs().max()) == 0.0 for k in DIST_KEYS)


@pytest.mark.parametrize("R,S,P", LC.INTER_CASES + [LC.INTER_LIMIT])
def test_interlevel_values_and_gradients(R, S, P):
    dev = _dev()
    for regime in LC.INTER_REGIMES:
        if not LC.interlevel_possible(S, P, regime):
            continue
        c = LC.interlevel_case(R, S, P, regime)
        name = f"interlevel R={R} S={S} P={P} {regime}"
        ref_loss, ref_grad, violated = c["ref"]
        # the condition, from the oracle, before the kernel is looked at: the case exercises the bound
        share = float(violated.double().mean())
        print(f"{name}: {100 * share:.1f} % of the cells have w_k > bound_k")
        assert share == 0.0 if regime == "covered" else share >= 0.10, f"{name}: {share}"
        loss, t = _interlevel(c, dev)
        grad = t["proposal_weights"].grad
        assert loss.shape == (R,) and grad.shape == (R, P) and all(t[k].grad is None for k in INTER_KEYS if k != "proposal_weights")
        if regime == "covered":
            assert float(loss.abs().max()) == 0.0 and float(grad.abs().max()) == 0.0, f"{name}: not exactly zero"
            continue
        _worst(f"{name} loss", loss, ref_loss)
        _worst(f"{name} d proposal_weights", grad, ref_grad)


def test_upstream_gradient_and_eps():
    """a loss gradient that is not ones, and an eps that is not the default, against the oracle with the same"""
    dev = _dev()
    c = LC.distortion_case(130, 131, "mixed")
    _, t = _distortion(c, dev, g=c["g"])
    ref = LC.distortion_oracle(c["weights"], c["depths"], c["deltas"], g=c["g"])
    for k, want in zip(DIST_KEYS, ref[1:]):
        _worst(f"distortion, upstream gradient: d {k}", t[k].grad, want)
    c = LC.interlevel_case(130, 131, 65, "violating")
    four = tuple(c[k] for k in INTER_KEYS)
    for eps in (1e-7, 1e-3):
        loss, t = _interlevel(c, dev, g=c["g"], eps=eps)
        ref_loss, ref_grad, _ = LC.interlevel_oracle(*four, eps=eps, g=c["g"])
        _worst(f"interlevel, upstream gradient, eps {eps}: loss", loss, ref_loss)
        _worst(f"interlevel, upstream gradient, eps {eps}: d proposal_weights", t["proposal_weights"].grad, ref_grad)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. partial gradients, grad_loss, reproducibility
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R,S", [(63, 1), (130, 65), (3, 2048)])
def test_partial_distortion_gradients_are_the_full_ones_bit_for_bit(R, S):
    dev = _dev()
    c = LC.distortion_case(R, S, "mixed")
    _, full = _distortion(c, dev, g=c["g"])
    for n in (1, 2):
        for subset in itertools.combinations(DIST_KEYS, n):
            _, t = _distortion(c, dev, requires_grad=subset, g=c["g"])
            for k in DIST_KEYS:
                if k in subset:
                    assert torch.equal(t[k].grad, full[k].grad), f"R={R} S={S}: d {k} of {subset} differs from the full run"
                else:
                    assert t[k].grad is None
    loss, t = _distortion(c, dev, requires_grad=())
    assert not loss.requires_grad


def test_grad_loss_omitted_means_ones():
    """the C entry points with grad_loss == NULL against a buffer of ones (bit for bit) and against other values"""
    dev = _dev()
    stream = _lib.current_stream(dev)
    c = LC.distortion_case(130, 65, "transparent")
    w, d, dl = (c[k].to(dev) for k in DIST_KEYS)
    R, S = w.shape
    runs = {}
    for key, g in (("omitted", None), ("ones", torch.ones(R, device=dev)), ("given", c["g"].to(dev))):
        grads = [torch.full_like(w, float("nan")) for _ in range(3)]
        a = _lib.LpDistortionArgs()
        a.n_rays, a.n_samples = R, S
        a.weights, a.depths, a.deltas, a.grad_loss = w.data_ptr(), d.data_ptr(), dl.data_ptr(), None if g is None else g.data_ptr()
        a.grad_weights, a.grad_depths, a.grad_deltas = (t.data_ptr() for t in grads)
        assert _lib.lib().lp_distortion_backward(ctypes.byref(a), stream) == 0
        torch.cuda.synchronize()
        runs[key] = grads
    for x, y, z in zip(runs["omitted"], runs["ones"], runs["given"]):
        assert torch.equal(x, y)
        assert torch.equal(z, c["g"].to(dev)[:, None] * x)  # (the kernel's last operation is this product)
    c = LC.interlevel_case(130, 131, 65, "violating")
    four = [c[k].to(dev) for k in INTER_KEYS]
    runs = {}
    for key, g in (("omitted", None), ("ones", torch.ones(130, device=dev)), ("given", c["g"].to(dev))):
        grad = torch.full_like(four[2], float("nan"))
        a = _lib.LpInterlevelArgs()
        a.n_rays, a.n_samples, a.n_proposal, a.eps = 130, 131, 65, LC.EPS
        a.weights, a.depths, a.proposal_weights, a.proposal_depths = (t.data_ptr() for t in four)
        a.grad_loss, a.grad_proposal_weights = None if g is None else g.data_ptr(), grad.data_ptr()
        assert _lib.lib().lp_interlevel_backward(ctypes.byref(a), stream) == 0
        torch.cuda.synchronize()
        runs[key] = grad
    assert torch.equal(runs["omitted"], runs["ones"])
    _worst("interlevel, grad_loss given vs g x omitted", runs["given"], c["g"][:, None].double() * runs["omitted"].double().cpu(), tol=1e-6)


def test_two_runs_are_bit_identical():
    dev = _dev()
    for key in ((130, 131, "transparent"), (63, 65, "mixed"), (3, 2048, "opaque")):
        c = LC.distortion_case(*key)
        runs = []
        for _ in range(2):
            loss, t = _distortion(c, dev, g=c["g"])
            runs.append((loss,) + tuple(t[k].grad for k in DIST_KEYS))
        assert all(torch.equal(a, b) for a, b in zip(*runs)), key
    for key in ((130, 131, 65, "violating"), (63, 64, 64, "duplicates"), (3, 2048, 2048, "disjoint")):
        c = LC.interlevel_case(*key)
        runs = []
        for _ in range(2):
            loss, t = _interlevel(c, dev, g=c["g"])
            runs.append((loss, t["proposal_weights"].grad))
        assert all(torch.equal(a, b) for a, b in zip(*runs)), key


# ------------------------------------------------------------------------------------------------------------------------------
# 3. hygiene
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", GA.PATTERNS)
def test_every_buffer_is_written_entirely(pattern):
    """forward and backward under poisoned, fenced allocations: no element of a result or a gradient keeps the poison and every fence is
    intact (checked when the block ends)"""
    dev = _dev()
    with GA.guarded(pattern) as g:
        for key in ((63, 1, "mixed"), (130, 65, "transparent"), (1, 131, "opaque"), (3, 2048, "duplicates")):
            c = LC.distortion_case(*key)
            _distortion(c, dev)
            _distortion(c, dev, requires_grad=("depths",))
        for key in ((63, 2, 3, "violating"), (130, 131, 65, "contains"), (1, 65, 65, "covered"), (3, 2048, 2048, "duplicates")):
            _interlevel(LC.interlevel_case(*key), dev)
        torch.cuda.synchronize()
        records = g.from_file("lightplane_amd/ray_losses.py")
        poisoned = [r for r in records if r.poisoned]
        assert len(poisoned) >= 4 * (1 + 3 + 1 + 1) + 4 * 2, len(poisoned)
        for r in poisoned:
            assert g.unwritten(r) == 0, f"{g.unwritten(r)} of {r.payload.numel()} elements unwritten: {r.where()}"


def test_empty_batch():
    dev = _dev()
    z = lambda *s: torch.zeros(*s, device=dev, requires_grad=True)  # noqa: E731
    w, d, dl = z(0, 5), z(0, 5), z(0, 5)
    loss = lp.distortion_loss(w, d, dl)
    assert loss.shape == (0,)
    loss.sum().backward()
    assert w.grad.shape == d.grad.shape == dl.grad.shape == (0, 5)
    pw = z(0, 7)
    loss = lp.interlevel_loss(w, d, pw, z(0, 7))
    assert loss.shape == (0,)
    loss.sum().backward()
    assert pw.grad.shape == (0, 7)
    torch.cuda.synchronize()


def test_memory_is_the_results():
    """a no-grad call allocates its result and (allocator rounding aside) nothing else; a backward its gradients and the contiguous
    upstream gradient: the bound of tests/test_gpu_compositing.py::test_memory_is_the_results"""
    dev = _dev()
    R, S = 4096, 128
    c = LC.distortion_inputs(R, S, "transparent")
    w, d, dl = (c[k].to(dev) for k in DIST_KEYS)
    ic = LC.interlevel_inputs(R, S, S, "violating")
    four = [ic[k].to(dev) for k in INTER_KEYS]

    def peak(fn, clear=lambda: None):
        fn()  # (library and kernels are loaded)
        clear()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        out = fn()
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated(dev) - before
        del out
        return extra

    with torch.no_grad():
        for name, fn in (("distortion_loss", lambda: lp.distortion_loss(w, d, dl)), ("interlevel_loss", lambda: lp.interlevel_loss(*four))):
            extra, results = peak(fn), 4 * R
            print(f"{name}: peak extra memory {extra} bytes for a result of {results}")
            assert extra <= 1.25 * results + 64 * 1024, f"{name}: {extra} bytes beyond the inputs for {results} bytes of results"
    leaves = [t.clone().requires_grad_(True) for t in (w, d, dl)]

    def clear():
        for t in leaves:
            t.grad = None

    def step():
        lp.distortion_loss(*leaves).sum().backward()
        return [t.grad for t in leaves]

    extra, results = peak(step, clear), 3 * 4 * R * S
    print(f"distortion_loss forward + backward: peak extra memory {extra} bytes for gradients of {results}")
    assert results <= extra <= 1.25 * results + 64 * 1024


def _warm_up(fn, times=1):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(times):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


def test_graph_capture_with_replay_on_new_weights():
    """forward + backward of both losses captured once on one stream and replayed on new weights: every replay equals the eager run on
    the same values to the bit"""
    dev = _dev()
    c = LC.distortion_case(130, 65, "transparent")
    ic = LC.interlevel_case(130, 131, 65, "violating")
    w, d, dl = (c[k].to(dev).clone().requires_grad_(True) for k in DIST_KEYS)
    tw, td, pw, pd = (ic[k].to(dev).clone() for k in INTER_KEYS)
    pw.requires_grad_(True)
    g = c["g"].to(dev)
    leaves = (w, d, dl, pw)

    def step():
        for t in leaves:
            t.grad = None
        a, b = lp.distortion_loss(w, d, dl), lp.interlevel_loss(tw, td, pw, pd)
        ((a * g).sum() + (b * g).sum()).backward()
        return a, b

    _warm_up(step, 3)
    for t in leaves:
        t.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    captured = [t.grad for t in leaves]
    first = None
    for round_ in range(2):
        if round_ == 1:  # new values in the tensors the graph reads
            with torch.no_grad():
                w.copy_(LC.distortion_case(130, 65, "opaque")["weights"].to(dev))
                pw.copy_(0.5 * ic["proposal_weights"].to(dev))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.detach().clone() for t in tuple(out) + tuple(captured)]
        eager = step()
        for i, (a, b) in enumerate(zip(replayed, tuple(eager) + tuple(t.grad for t in leaves))):
            assert torch.equal(a, b.detach()), f"round {round_}: replayed tensor {i} != eager"
        if round_ == 0:
            first = [t.clone() for t in replayed[:2]]
    assert all(float((a - b).abs().max()) > 1e-4 for a, b in zip(replayed[:2], first))  # (the second round really saw other weights)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the chains, the example
# ------------------------------------------------------------------------------------------------------------------------------

def test_the_chain_to_the_distortion_loss_with_gradients_into_the_grids():
    """ray_samples -> lightplane_eval_mlp -> composite_samples(return_weights) -> distortion_loss, against the same chain in fp64:
    the oracle's sample placement, decoder and compositing (tests/compositing_cases.py) and the pair form of the loss"""
    from oracle import lightplane_oracle as O
    from tests import compositing_cases as CC
    dev, c = _dev(), CC.chain_case("triplane")
    r = c["rays"]
    rays = lp.Rays(grid_idx=r.grid_idx.to(dev), encoding=r.encoding.to(dev), origins=r.origins.to(dev), directions=r.directions.to(dev),
                   near=r.near.to(dev), far=r.far.to(dev))
    grids = [g.to(dev).requires_grad_(True) for g in c["grids"]]
    dec = lp.DecoderParams(c["dec"].mlp_params.to(dev).requires_grad_(True), c["dec"].n_hidden_trunk, c["dec"].n_hidden_opacity, c["dec"].n_hidden_color, 3)
    up = c["ups"][0]
    s = lp.ray_samples(rays, CC.CHAIN_S, CC.CHAIN_S_INF, disparity_at_inf=CC.CHAIN_DISPARITY)
    opacity, color = lp.lightplane_eval_mlp(s.points, grids, rays.grid_idx, dec, rays.encoding, CC.CHAIN_GAIN, contract_coords=c["contract"])
    weights = lp.composite_samples(opacity, color, s.depths, s.deltas, return_weights=True)[3]
    loss = lp.distortion_loss(weights, s.depths, s.deltas)
    (loss * up.to(dev)).sum().backward()

    p64 = c["dec"].mlp_params.double().requires_grad_(True)
    dec64 = lp.DecoderParams(p64, dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, 3)
    g64 = [g.double().requires_grad_(True) for g in c["grids"]]
    r64 = lp.Rays(directions=r.directions.double(), origins=r.origins.double(), grid_idx=r.grid_idx, near=r.near.double(), far=r.far.double(),
                  encoding=r.encoding.double())
    points, depths, deltas = CC.placement(r64, CC.CHAIN_S, CC.CHAIN_S_INF, CC.CHAIN_DISPARITY, torch.float64)
    o64, c64 = O.eval_decoder(points, g64, r.grid_idx, dec64, r64.encoding, CC.CHAIN_GAIN, contract_coords=c["contract"])
    w64 = CC.composite(o64, c64[..., :3], depths, deltas)[3]
    ref = LC.distortion_pairs(w64, depths, deltas)
    (ref * up.double()).sum().backward()
    _worst("chain -> distortion loss", loss, ref.detach())
    assert float(ref.detach().abs().max()) > 1e-4
    for i, (g, want) in enumerate(zip(grids, g64)):
        _worst(f"chain -> distortion d grid[{i}]", g.grad, want.grad)
    _worst("chain -> distortion d mlp_params", dec.mlp_params.grad, p64.grad)


def test_the_coarse_to_fine_chain_to_the_interlevel_loss():
    """coarse march -> importance_samples -> fine march, interlevel_loss(w_fine, d_fine, w_coarse, d_coarse) and its gradient to the
    coarse weights (and through them to a parameter of the coarse density), against the oracle on the kernels' own tensors"""
    dev = _dev()
    R = 130
    gen = torch.Generator().manual_seed(5)
    origins = torch.tensor([0.0, 0.0, -2.5]) + 0.05 * torch.randn(R, 3, generator=gen)
    directions = torch.nn.functional.normalize(torch.tensor([0.0, 0.0, 1.0]) + 0.08 * torch.randn(R, 3, generator=gen), dim=-1)
    rays = lp.Rays(directions=directions.to(dev), origins=origins.to(dev), grid_idx=torch.zeros(R, dtype=torch.long, device=dev),
                   near=torch.full((R,), 1.0, device=dev), far=torch.full((R,), 4.0, device=dev))
    scale = torch.full((R, 1), 0.05, device=dev, requires_grad=True)  # the coarse ("proposal") density underestimates the scene

    def density(p):  # a soft ball of radius 0.5
        return 20.0 * torch.sigmoid(40.0 * (0.5 - p.norm(dim=-1)))

    coarse = lp.ray_samples(rays, 32)
    w_coarse = lp.composite_samples(scale * density(coarse.points), None, coarse.depths, coarse.deltas, return_weights=True)[3]
    w_coarse.retain_grad()
    fine = lp.importance_samples(rays, coarse.depths, w_coarse, 33)
    w_fine = lp.composite_samples(density(fine.points), None, fine.depths, fine.deltas, return_weights=True)[3]
    assert fine.depths.shape == (R, 65) and w_fine.shape == (R, 65)
    loss = lp.interlevel_loss(w_fine, fine.depths, w_coarse, coarse.depths)
    loss.sum().backward()
    four = tuple(t.detach().cpu() for t in (w_fine, fine.depths, w_coarse, coarse.depths))
    ref_loss, ref_grad, violated = LC.interlevel_oracle(*four)
    print(f"coarse -> fine: {100 * float(violated.double().mean()):.1f} % of the cells have w_k > bound_k")
    assert float(ref_loss.max()) > 1e-3 and float(ref_grad.abs().max()) > 1e-3  # (the proposal is violated: there is something to compare)
    _worst("coarse -> fine interlevel loss", loss, ref_loss)
    _worst("coarse -> fine d coarse weights", w_coarse.grad, ref_grad)
    assert bool(torch.isfinite(scale.grad).all()) and float(scale.grad.abs().max()) > 0  # (and on through the coarse march)


def test_example_fits_with_the_distortion_loss():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "fit_synthetic_scene.py"), "--modular", "--importance", "32",
                        "--distortion-weight", "0.01", "--steps", "20", "--rays", "2048"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = r.stdout.decode()
    assert r.returncode == 0, text
    out = json.loads(text.strip().splitlines()[-1])
    print(out)
    assert out["modular"] is True and out["importance"] == 32 and out["distortion_weight"] == 0.01 and out["steps"] == 20, out
    assert out["last_loss"] < out["first_loss"] and out["first_distortion"] > 0 and out["last_distortion"] > 0, out

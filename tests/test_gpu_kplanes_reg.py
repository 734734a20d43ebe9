"""The fused K-Planes regularisers (lightplane_amd/regularizers.py, csrc/lp_kplanes_reg.hip) against their definition: ``reference``
below, torch fp64 on the CPU on the fp32 inputs, slices + autograd.  Bar, as tests/test_gpu_grid_tv.py and tests/test_gpu_kplanes.py
have it: max |err| / max |ref| <= 1e-4 per term and per gradient tensor, exact zeros where the definition gives exact zeros.
Measured worst errors (this file's cases, MI355X): 5.3e-8 on a term, 2.4e-7 on grad_planes, 2.6e-7 on the accumulated gradient
(DESIGN.md 4.28)."""
import json
import os
import subprocess
import sys

import pytest
import torch

import lightplane_amd as lp
from tests.test_gpu_kplanes import DYN
from tests.test_gpu_parity import _dev
from tests.test_gpu_ray_grid import _worst   # max |err| / max |ref|, printed before it is held to the bar

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
LAYOUTS = {
    "dynamic": DYN,
    "static": dict(DYN, time_resolution=None),
    "c4": dict(DYN, channels=4),
    "c64": dict(DYN, channels=64),
    "min_res": dict(resolutions=(2,), time_resolution=(2,), channels=8),     # no triple, one pair per axis
    "one_triple": dict(DYN, time_resolution=(3, 3)),
    "kplanes_128": dict(resolutions=(4, 8, 16, 32), time_resolution=6, channels=32),   # a table of 24 planes
    # C = 64: a strip is 256 / 16 = 16 vertices, a chunk 32 rows (KR_VC): n_u = 37 = 2 strips + 5, n_v = 37 = 1 chunk + 5 on the space
    # planes and 71 = 2 chunks + 7 on the space-time planes -- strip edges, chunk edges and the halo rows of the 5-point stencil
    "edges": dict(resolutions=(37,), time_resolution=(71,), channels=64),
}


def _planes_of(planes, lay):
    """(view [B, n_v, n_u, C], is a space-time plane) of every plane"""
    for s in range(lay.n_scales):
        for j in range(lay.n_planes):
            n_u, n_v = lay.spatial[s], lay.spatial[s] if j < 3 else lay.temporal[s]
            off = lay.offsets[s][j]
            yield planes[:, off:off + n_u * n_v].view(planes.shape[0], n_v, n_u, -1), j >= 3


def reference(planes, lay, p):
    """the definition: (space_tv, time_smoothness, time_l1) as a [3] tensor in the dtype of ``planes``"""
    phi = torch.abs if p == 1 else torch.square
    tv, smooth, l1 = (planes.new_zeros(()) for _ in range(3))
    for X, is_time in _planes_of(planes, lay):
        tv = tv + phi(X[:, :, 1:] - X[:, :, :-1]).mean()
        if not is_time:
            tv = tv + phi(X[:, 1:] - X[:, :-1]).mean()
            continue
        if X.shape[1] > 2:
            smooth = smooth + (X[:, 2:] - 2 * X[:, 1:-1] + X[:, :-2]).square().mean()
        l1 = l1 + (1 - X).abs().mean()
    return torch.stack([tv, smooth, l1])


def _field(lay, B, seed):
    return torch.rand(B, lay.rows, lay.channels, generator=torch.Generator().manual_seed(seed)) * 2.0


@pytest.mark.parametrize("B", (1, 2))
@pytest.mark.parametrize("p", (1, 2))
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_terms_and_gradients_against_the_definition(name, p, B):
    dev, lay = _dev(), lp.kplanes_layout(**LAYOUTS[name])
    host = _field(lay, B, 2800 + len(name))
    up = torch.tensor([0.7, -1.3, 2.1])
    ref_in = host.double().requires_grad_()
    want = reference(ref_in, lay, p)
    (want_grad,) = torch.autograd.grad((want * up.double()).sum(), ref_in)
    planes = host.to(dev).requires_grad_()
    terms = lp.kplanes_regularizers(planes, lay, p=p)
    (grad,) = torch.autograd.grad(terms, planes, up.to(dev))
    for k, term in enumerate(("space_tv", "time_smoothness", "time_l1")):
        if float(want[k].detach()) == 0.0:
            assert float(terms[k]) == 0.0, term
        else:
            _worst(f"{name} p={p} B={B} {term}", terms[k], want[k], tol=TOL)
    _worst(f"{name} p={p} B={B} grad_planes", grad, want_grad, tol=TOL)
    # the fused accumulate on a buffer that starts at the gradient's own magnitude
    w = (0.5, 1.5, -2.0)
    (want_w,) = torch.autograd.grad((reference(ref_in, lay, p) * torch.tensor(w).double()).sum(), ref_in)
    start = (torch.rand(host.shape, generator=torch.Generator().manual_seed(7)) - 0.5) * float(want_w.abs().max())
    buf, before = start.to(dev), planes.detach().clone()
    fused = lp.add_kplanes_reg_grad_(planes.detach(), buf, lay, weights=w, p=p)
    assert torch.equal(fused, terms) and torch.equal(planes.detach(), before)
    _worst(f"{name} p={p} B={B} accumulated - start", buf.double().cpu() - start.double(), want_w, tol=TOL)


@pytest.mark.parametrize("p", (1, 2))
def test_exact_zeros_of_a_fresh_field_and_of_ties(p):
    dev, lay = _dev(), lp.kplanes_layout(**DYN)
    planes = lp.init_kplanes(lay, 2, device=dev).requires_grad_()
    terms = lp.kplanes_regularizers(planes, lay, p=p)
    assert terms.detach().cpu().gt(0).tolist() == [True, False, False]
    (grad,) = torch.autograd.grad(terms, planes, torch.tensor([0.0, 1.0, 1.0], device=dev))
    assert not grad.any()        # the two time terms give nothing anywhere, and the space term was not asked
    (grad,) = torch.autograd.grad(lp.kplanes_regularizers(planes, lay, p=p), planes, torch.ones(3, device=dev))
    for X, is_time in _planes_of(grad, lay):
        assert bool(X.any()) != is_time     # constant planes: every difference is a tie
    # runs of equal neighbours: rows of u are constant, so the p = 1 gradient along u is exactly 0 there
    steps = torch.arange(lay.rows, device=dev).float()[None, :, None].expand(1, lay.rows, lay.channels).contiguous()
    for X, _ in _planes_of(steps, lay):
        X[:] = X[:, :, :1].clone()
    buf = torch.zeros_like(steps)
    lp.add_kplanes_reg_grad_(steps, buf, lay, weights=(1.0, 0.0, 0.0), p=1)
    for X, is_time in _planes_of(buf, lay):
        if is_time:
            assert not X.any()
        else:                    # the v axis rises: -1 / N on the first row, +1 / N on the last, ties (0) between
            assert bool((X[:, 0] < 0).all()) and bool((X[:, -1] > 0).all()) and not X[:, 1:-1].any()


def test_no_pair_crosses_a_plane_a_scene_or_a_row():
    dev, lay = _dev(), lp.kplanes_layout(**DYN)
    host = _field(lay, 2, 41)
    base = lp.kplanes_regularizers(host.to(dev), lay).cpu()
    # a constant offset on one whole plane, and on one whole scene: first and second differences inside it do not change
    moved = host.clone()
    off, n = lay.offsets[1][1], lay.spatial[1] ** 2
    moved[0, off:off + n] += 1000.0
    moved[1] += 1000.0
    got = lp.kplanes_regularizers(moved.to(dev), lay).cpu()
    want = reference(moved.double(), lay, 2)
    assert ((got[:2] - base[:2]).abs() <= 1e-2 * base[:2]).all()    # (fp32 differences of values near 1000)
    for k in range(3):
        _worst(f"offset plane and scene, term {k}", got[k], want[k], tol=TOL)
    # a field that is linear along u within every row of every plane: every u-pair is exactly 1, whatever the row before holds
    ramp = torch.zeros(1, lay.rows, lay.channels)
    for X, _ in _planes_of(ramp, lay):
        X += torch.arange(X.shape[2]).float()[None, None, :, None]
    got = lp.kplanes_regularizers(ramp.to(dev), lay, p=1).cpu()
    assert float(got[0]) == float(lay.n_scales * lay.n_planes) and float(got[1]) == 0.0


def test_reproducible_and_graph_capturable():
    dev, lay = _dev(), lp.kplanes_layout(**LAYOUTS["kplanes_128"])
    w = (0.5, 1.5, 2.0)
    planes = _field(lay, 2, 5).to(dev)
    runs = []
    for _ in range(2):
        buf = torch.zeros_like(planes)
        runs.append((lp.add_kplanes_reg_grad_(planes, buf, lay, weights=w, p=1), buf))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    buf = torch.zeros_like(planes)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            lp.add_kplanes_reg_grad_(planes, buf, lay, weights=w, p=1)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):      # a single chain: the sweep, then the finish
        terms = lp.add_kplanes_reg_grad_(planes, buf, lay, weights=w, p=1)
    for seed in (6, 7):                # replayed on new contents of the same memory
        planes.copy_(_field(lay, 2, seed))
        eager = torch.zeros_like(planes)
        eager_terms = lp.add_kplanes_reg_grad_(planes, eager, lay, weights=w, p=1)
        buf.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(terms, eager_terms) and torch.equal(buf, eager)


def test_fit_synthetic_scene_kplanes_with_tv_weight():
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "fit_synthetic_scene.py"), "--modular", "--kplanes", "--steps", "10",
                        "--rays", "1024", "--tv-weight", "1e-3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["kplanes"] is True and out["tv_weight"] == 1e-3
    for k in ("first_loss", "last_loss", "first_space_tv", "last_space_tv"):
        assert out[k] == out[k] and abs(out[k]) < float("inf"), k
    assert out["first_space_tv"] > 0.0

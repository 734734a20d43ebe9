"""The shape-generic kernels at ragged widths (tests/ragged_cases.py) against the fp64 oracle.

Renderer: outputs at the project's 1e-4 against the plain fp64 oracle, and the proof of ``forced_oracle_check`` -- the backward's own
ReLU decisions, read back from the DUMP twin of the generic kernel, forced onto the fp64 oracle, every forced unit a near tie, every
entry of every output and gradient at 1e-4 outright -- once with every gradient requested and once without ``grad_mlp_params`` (no
``wave_outer``, LDS_ACC off, the matrix-core input gradient still on).  The counted ReLU-flip allowance is not used in this file.
MLP-Splatter: ``forced_oracle_check_mlp_splatter`` on both kernel settings.  Plain Splatter: ``_check_splatter_all`` of the sweep, and
``lp_splatter_normalize`` on its own.  The ray embedding, the point evaluation and the scaffold take their ragged rows in their own
files (tests/test_gpu_modules.py, tests/points_cases.py, tests/test_gpu_scaffold.py)."""
import copy
import warnings

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib
from lightplane_amd.renderer import relu_dump_recorder
from oracle import lightplane_oracle as O
from tests import ragged_cases as R
from tests.test_gpu_parity import (FORCED_EVENTS, FORCED_TIE_K, KERNEL_IDS, KERNELS, REL_TOL, TIE_EPS, _assert_close, _dev, _rays_to, _rel_err,
                                   forced_oracle_check, forced_oracle_check_mlp_splatter, has_dump_twin, oracle_forced)
from tests.test_gpu_sweep import _check_splatter_all

pytestmark = pytest.mark.gpu

F64 = torch.float64
_BUILT = {}   # case name -> (inputs, fp64 oracle outputs); computed once, never modified


def _built(case):
    if case.name not in _BUILT:
        d = case.build()
        rays = copy.copy(d["rays"])
        for f in ("directions", "origins", "near", "far", "encoding"):
            setattr(rays, f, getattr(rays, f).to(F64))
        dec = copy.copy(d["decoder"])
        dec.mlp_params = dec.mlp_params.to(F64)
        with torch.no_grad():
            o64 = O.lightplane_renderer_naive(rays, [g.to(F64) for g in d["grids"]], dec,
                                              scaffold=None if d["scaffold"] is None else d["scaffold"].to(F64),
                                              color_grid=None if d["color_grids"] is None else [g.to(F64) for g in d["color_grids"]], **d["cfg"])
        _BUILT[case.name] = (d, o64)
    return _BUILT[case.name]


def _run_without_param_grads(d, dev):
    """tests.test_gpu_parity.run_hip_renderer with ``mlp_params`` not requiring a gradient: the front-end hands the library a NULL
    ``grad_mlp_params``"""
    rays = _rays_to(d["rays"], dev, True)
    dec = d["decoder"]
    params = dec.mlp_params.to(dev).clone()
    hdec = lp.DecoderParams(params, dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
    grids = [g.to(dev).clone().requires_grad_(True) for g in d["grids"]]
    cgrids = None if d["color_grids"] is None else [g.to(dev).clone().requires_grad_(True) for g in d["color_grids"]]
    scaffold = None if d["scaffold"] is None else d["scaffold"].to(dev)
    out = lp.lightplane_renderer(rays, grids, hdec, scaffold=scaffold, color_grid=cgrids, kernel=_lib.LP_KERNEL_AUTO, **d["cfg"])
    g_len, g_nlt, g_feat = (t.to(dev) for t in d["upstream"])
    ((out[0] * g_len).sum() + (out[1] * g_nlt).sum() + (out[2] * g_feat).sum()).backward()
    assert params.grad is None
    return out, rays.encoding.grad, [g.grad for g in grids], None if cgrids is None else [g.grad for g in cgrids]


def _forced_check_without_param_grads(name, d, dev):
    """``forced_oracle_check`` for the launch without ``grad_mlp_params``: the same bounds on the forcing, the same 1e-4 on every
    output and every gradient that was asked for."""
    prod = _run_without_param_grads(d, dev)
    with relu_dump_recorder() as rec:
        twin = _run_without_param_grads(d, dev)
    assert rec.dump is not None, "the backward did not go through the dump hook"
    pairs = [("grad_encoding", prod[1], twin[1])] + [(f"grad_grid{i}", a, b) for i, (a, b) in enumerate(zip(prod[2], twin[2]))]
    pairs += [(f"grad_color_grid{i}", a, b) for i, (a, b) in enumerate(zip(prod[3] or [], twin[3] or []))]
    for nm, a, b in pairs:
        e = float((a - b).abs().max()) / (float(a.abs().max()) + 1e-30)
        assert e <= 2e-5, f"dump twin vs production launch: {nm} differs by {e:.3e}"
    out, ge, gg, gc = prod
    f_out, _, f_ge, f_gg, f_gc, st = oracle_forced(d, rec.dump, None, chunk=d["rays"].n_rays, words_per_site=rec.words_per_site)
    worst = {}
    for nm, a, b in [("ray_length", out[0], f_out[0]), ("neg_log_t", out[1], f_out[1]), ("feature", out[2], f_out[2]), ("grad_encoding", ge, f_ge)] + \
            [(f"grad_grid{i}", a, b) for i, (a, b) in enumerate(zip(gg, f_gg))] + \
            [(f"grad_color_grid{i}", a, b) for i, (a, b) in enumerate(zip(gc or [], f_gc or []))]:
        worst[nm] = _rel_err(a, b.numpy())
    FORCED_EVENTS.append(dict(name=name, forced_units=st["n_forced"], visited_samples=int((rec.dump[..., -1] != 0).sum()),
                              max_forced_margin=float(f"{st['max_forced_margin']:.3e}"), near_tie_units=st["n_near_units"], units=st["n_units"],
                              worst={k: float(f"{v:.3e}") for k, v in worst.items()}))
    print(f"forced-oracle {name}: {st['n_forced']} ReLU units forced (largest margin {st['max_forced_margin']:.2e}, {st['n_near_units']} near-tie "
          f"units in the oracle); max err / scale: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert st["max_forced_margin"] <= FORCED_TIE_K * TIE_EPS, f"{name}: a forced unit is not a near tie ({st['max_forced_margin']:.3e})"
    assert st["n_forced"] <= st["n_near_units"], f"{name}: {st['n_forced']} forced units, {st['n_near_units']} near-tie units in the fp64 oracle"
    bad = {k: v for k, v in worst.items() if not v <= REL_TOL}
    assert not bad, f"{name}: with the kernel's own ReLU decisions forced onto the fp64 oracle these still miss {REL_TOL:g}: {bad}"
    return out


@pytest.mark.parametrize("want_params", [True, False], ids=["all_gradients", "no_grad_mlp_params"])
@pytest.mark.parametrize("case", R.RENDERER_CASES, ids=lambda c: c.name)
def test_renderer_at_ragged_widths(case, want_params):
    dev = _dev()
    d, o64 = _built(case)
    assert lp.kernel_family(d["rays"], d["grids"], d["decoder"], color_grid=d["color_grids"]) == 0
    assert has_dump_twin(d), "the shape-generic backward has a dump twin"
    with warnings.catch_warnings():
        # the shape-generic kernels are what is under test here: their "10-100x slower" warning is expected
        warnings.filterwarnings("ignore", message=".*shape-generic Renderer kernels", category=UserWarning)
        if want_params:
            _, prod, _ = forced_oracle_check(f"ragged {case.name}", d, dev, chunk=case.n_rays, return_results=True)
            out = prod[0]
        else:
            out = _forced_check_without_param_grads(f"ragged {case.name} [no grad_mlp_params]", d, dev)
    for nm, a, b in zip(("ray_length", "neg_log_t", "feature"), out, o64):
        print(f"ragged {case.name} {nm}: {_rel_err(a, b.numpy()):.3e} against the fp64 oracle")
        _assert_close(f"{case.name}: {nm} / fp64 oracle", a, b.numpy(), REL_TOL)


@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("case", R.MLP_SPLATTER_CASES, ids=lambda c: c.name)
def test_mlp_splatter_at_ragged_widths(case, kernel):
    forced_oracle_check_mlp_splatter(f"ragged mlp-splatter {case.name} [{KERNEL_IDS[KERNELS.index(kernel)]}]", case.build(), _dev(), kernel=kernel)


@pytest.mark.filterwarnings("ignore:The splatter has been configured")
@pytest.mark.parametrize("case", R.SPLATTER_CASES, ids=lambda c: c.name)
def test_splatter_at_ragged_channel_counts(case):
    _check_splatter_all(case, case.name, case.build(), _dev())


@pytest.mark.parametrize("C", R.NORMALIZE_CHANNELS)
def test_splatter_normalize_at_ragged_channel_counts(C):
    """``lp_splatter_normalize`` alone against feat / clamp(weight, 1e-5): rows nothing was splatted into (feature and weight 0), rows
    whose weight is below the clamp, 1 003 rows (the last block is partial)."""
    dev = _dev()
    gen = torch.Generator().manual_seed(40 + C)
    rows = 1003
    weight = torch.rand(rows, generator=gen) * 2
    weight[::4] = 0.0
    weight[1::16] *= 4e-6  # below the clamp
    feat = torch.randn(rows, C, generator=gen) * weight[:, None]
    want = feat.double() / weight.double().clamp(min=1e-5)[:, None]
    got, w = feat.to(dev).contiguous(), weight.to(dev)
    _lib.check(_lib.lib().lp_splatter_normalize(got.data_ptr(), w.data_ptr(), rows, C, _lib.current_stream(dev)), "lp_splatter_normalize")
    torch.cuda.synchronize()
    assert bool((want[1::16].abs().max() > 0)) and float(want[::4].abs().max()) == 0.0
    _assert_close(f"normalize C={C}", got, want.numpy(), REL_TOL)
    assert torch.equal(w.cpu(), weight)

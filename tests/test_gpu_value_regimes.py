"""Every copy of the compositing arithmetic -- ``softplus_f`` / ``__expf`` / ``sigmoid_f`` / ``nlt_add`` and the backward's -log T
reconstruction -- in the value regimes of tests/value_regime_cases.py, against the fp64 oracle.

Carriers: the 17 launches of tests/partial_grad_cases.py (each with its ``config``, ``kernel``, ``march_order``, ``flat``) in ``init``,
``surface``, ``extremes`` and ``opaque_late``; three of them with ``far == near`` on every fourth ray; the forward of deep hidden-64
decoders (resident and streamed weight images, shape-generic backward), the evaluation at points (lp_points.hip) and the scaffold's opacity
lattice (lp_scaffold.hip) in ``init`` / ``surface`` / ``extremes``.  tests/test_value_regimes_host.py proves without a GPU that every pair
reaches its regime and that the fp32 oracle meets the fp64 oracle at 2e-5 there.

Bars, the project's own: outputs and every gradient tensor at 1e-4 of the tensor's largest entry against the fp64 oracle with the
backward's own ReLU decisions forced onto it (``forced_oracle_check``: every forced unit a near tie, no more forced units than near ties);
the launches without a dump twin (``tuned_nw8``, ``tuned_fp32``) through ``assert_grad_close`` as in tests/test_gpu_partial_grads.py, every
use of its counted allowance printed; outputs against the plain fp64 oracle at 1e-4 outright; no NaN or Inf anywhere."""
import pytest
import torch

import lightplane_amd as lp
from tests import partial_grad_cases as T
from tests import points_cases as PC
from tests import value_regime_cases as V
from tests.test_gpu_parity import FLIP_EVENTS, FORCED_EVENTS, REL_TOL, _assert_close, _dev, _rel_err
from tests.test_gpu_partial_grads import ALL, LAST_BACKWARD, _baseline_meets_the_oracle, _last_backward, run_renderer
from tests.test_gpu_points import _joint, _opacity_only, _worst

pytestmark = pytest.mark.gpu

NAMES = ("ray_length", "neg_log_t", "feature")


def _tensors(base):
    return [(n, t) for n, t in zip(NAMES, base["out"])] + [("grad_mlp_params", base["P"]), ("grad_encoding", base["E"])] + \
        [(f"grad_grid{i}", g) for i, g in enumerate(base["G"])] + [(f"grad_color_grid{i}", g) for i, g in enumerate(base["Cg"] or [])]


def _hold_to_the_oracle(e, d, tag, forward_family=None, against_fp32=False):
    """One launch of the carrier (every leaf requiring a gradient) under the bars of the module docstring.  Returns its results."""
    dev = _dev()
    sel = T.renderer_selection(e, d)
    assert (sel["family"], sel["segments"]) == (e.family, e.segments), (tag, sel)
    if forward_family is not None:
        with T.config_set(**e.config):
            assert lp.forward_kernel_family(d["rays"], d["grids"], d["decoder"], color_grid=d["color_grids"],
                                            num_samples_inf=d["cfg"]["num_samples_inf"]) == forward_family, tag
    base = run_renderer(e, d, dev, ALL)
    assert LAST_BACKWARD[(sel["family"], sel["march"])] in _last_backward(), f"{tag}: the backward that ran is {_last_backward()}"
    for nm, t in _tensors(base):
        assert bool(torch.isfinite(t).all()), f"{tag}: {nm} holds {int((~torch.isfinite(t)).sum())} entries that are not finite"
    g64 = V.oracle_gradients(d)
    o64 = g64[0]
    for nm, a, b in zip(NAMES, base["out"], o64):
        print(f"value-regime {tag} {nm}: {_rel_err(a, b.numpy()):.3e} against the plain fp64 oracle")
        _assert_close(f"{tag}: {nm} / fp64 oracle", a, b.numpy(), REL_TOL)
    plain = [("grad_mlp_params", base["P"], g64[1]), ("grad_encoding", base["E"], g64[2])] + \
        [(f"grad_grid{i}", a, b) for i, (a, b) in enumerate(zip(_grid_list(e, d, base), g64[3]))] + \
        [(f"grad_color_grid{i}", a, b) for i, (a, b) in enumerate(zip(base["Cg"] or [], g64[4] or []))]
    print(f"value-regime {tag} gradients against the plain fp64 oracle (ReLU ties not forced): "
          + ", ".join(f"{nm} {_rel_err(a, b.numpy()):.2e}" for nm, a, b in plain))
    if against_fp32:
        g32 = V.oracle_gradients(d, torch.float32)
        pairs32 = [("grad_mlp_params", base["P"], g32[1]), ("grad_encoding", base["E"], g32[2])] + \
            [(f"grad_grid{i}", a, b) for i, (a, b) in enumerate(zip(_grid_list(e, d, base), g32[3]))] + \
            [(f"grad_color_grid{i}", a, b) for i, (a, b) in enumerate(zip(base["Cg"] or [], g32[4] or []))]
        print(f"value-regime {tag} gradients against the plain fp32 oracle: " + ", ".join(f"{nm} {_rel_err(a, b.numpy()):.2e}" for nm, a, b in pairs32))
    n_flip, n_forced = len(FLIP_EVENTS), len(FORCED_EVENTS)
    _baseline_meets_the_oracle(e, d, dev, base, tag=f"value-regime {tag}")
    for ev in FORCED_EVENTS[n_forced:]:
        print(f"value-regime {tag} forced units: {ev['forced_units']} of {ev['near_tie_units']} near ties; worst {max(ev['worst'].values()):.3e} "
              f"({max(ev['worst'], key=ev['worst'].get)})")
    for ev in FLIP_EVENTS[n_flip:]:
        print(f"value-regime {tag} COUNTED ALLOWANCE used: {ev['name']}: {ev['unexplained']} entries unexplained of {ev['allowed']} allowed")
    return base


def _grid_list(e, d, base):
    """the grid gradients per grid tensor, whatever form the carrier hands them over in"""
    if not e.flat:
        return base["G"]
    rows = [g.numel() // g.shape[-1] for g in d["grids"]]
    return [p.reshape(g.shape) for p, g in zip(base["G"][0].split(rows, dim=0), d["grids"])]


@pytest.mark.parametrize("entry_id,regime", V.RENDERER_PAIRS, ids=[f"{i}-{r}" for i, r in V.RENDERER_PAIRS])
def test_renderer_in_value_regime(entry_id, regime):
    e, d = V.built_renderer(entry_id, regime)
    _hold_to_the_oracle(e, d, f"{entry_id} [{regime}]", against_fp32=regime == "init")


@pytest.mark.parametrize("entry_id", V.ZERO_SPAN_ENTRIES)
def test_renderer_with_zero_span_rays(entry_id):
    """far == near on every fourth ray: the oracle's w is 0 on every sample of such a ray -- zero outputs, a zero row of grad_encoding --
    and the kernels give exactly that; everything else is held as in every regime."""
    e, d = V.built_renderer(entry_id, "zero_span")
    base = _hold_to_the_oracle(e, d, f"{entry_id} [zero_span]")
    flat = (d["rays"].far == d["rays"].near).to(base["E"].device)
    assert int(flat.sum()) == (T.N_RAYS + 3) // 4
    for nm, o in zip(NAMES, base["out"]):
        assert float(o[flat].abs().max()) == 0.0, f"{entry_id}: {nm} of a ray with far == near is {float(o[flat].abs().max()):.3e}"
    assert float(base["E"][flat].abs().max()) == 0.0, f"{entry_id}: grad_encoding of a ray with far == near is not zero"
    assert float(base["E"][~flat].abs().max()) > 0.0


@pytest.mark.parametrize("entry_id,regime", V.DEEP_PAIRS, ids=[f"{i}-{r}" for i, r in V.DEEP_PAIRS])
def test_deep_forward_in_value_regime(entry_id, regime):
    e, d = V.built_deep(entry_id, regime)
    _hold_to_the_oracle(e, d, f"{entry_id} [{regime}]", forward_family=V.DEEP_FORWARD_FAMILY[entry_id], against_fp32=regime == "init")


@pytest.mark.parametrize("name,regime", V.POINTS_PAIRS, ids=[f"{n}-{r}" for n, r in V.POINTS_PAIRS])
def test_points_in_value_regime(name, regime):
    """tests/test_gpu_points.py::test_values and ::test_gradients on the regime's decoder: the same points left out and zeroed."""
    dev, c = _dev(), V.points_case(name, regime)
    tag = f"points {name} [{regime}]"
    d = PC.on_device(c, dev, requires_grad=("points", "params", "enc", "grids", "cgrids"))
    op, col = _joint(d, c)
    assert bool(torch.isfinite(op).all()) and bool(torch.isfinite(col).all()), f"{tag}: a result is not finite"
    keep = ~c["left_out"]
    _worst(f"{tag} opacity", op, c["op"], keep)
    _worst(f"{tag} colour", col, c["col"], keep)
    with torch.no_grad():
        assert torch.equal(_opacity_only(d, c), op), "the opacity-only call and the joint call's opacity differ"
    ((op * c["u_op"].to(dev)).sum() + (col * c["u_col"].to(dev)).sum()).backward()
    gr = c["grads"]
    as_list = lambda g: g if isinstance(g, list) else [g]  # noqa: E731
    got = [(f"d grid[{i}]", t.grad, w) for i, (t, w) in enumerate(zip(as_list(d["grid"]), PC.flat_grad(c, gr["grids"])))]
    got += [("d mlp_params", d["params"].grad, gr["params"]), ("d rays_encoding", d["enc"].grad, gr["enc"]), ("d points", d["pts"].grad, gr["points"])]
    for nm, g, want in got:
        assert bool(torch.isfinite(g).all()), f"{tag} {nm}: not finite"
        _worst(f"{tag} {nm}", g, want)


@pytest.mark.parametrize("regime", list(V.SCAFFOLD_CONSTANTS))
def test_scaffold_opacity_in_value_regime(regime):
    """``scaffold_opacity`` against the oracle's ``gain * softplus`` on the lattice: on the series branch everywhere (``init``), across the
    overflow and the underflow of ``__expf`` (``extremes``)"""
    dev, c = _dev(), V.scaffold_case(regime)
    dec = c["dec"]
    ddec = lp.DecoderParams(dec.mlp_params.to(dev), dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
    assert c["form"] == "list"
    got = lp.scaffold_opacity([g.to(dev) for g in c["grids"]], ddec, c["size"], gain=c["gain"], mask_out_of_bounds_samples=c["mask"])
    assert got.shape == tuple(c["size"]) and bool(torch.isfinite(got).all())
    print(f"value-regime scaffold [{regime}]: worst |err| / max |ref| = {_rel_err(got, c['op'].numpy()):.3e} (max |ref| {float(c['op'].max()):.4g})")
    _assert_close(f"scaffold opacity lattice [{regime}]", got, c["op"].numpy(), tol=REL_TOL)

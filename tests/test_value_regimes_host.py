"""CPU tests of the value-regime tables (tests/value_regime_cases.py): every (carrier, regime) pair reaches what its regime promises in
the fp64 oracle (the ledger), stays on its carrier's kernel family and segment count, and is well conditioned -- the fp32 oracle agrees
with the fp64 oracle at 2e-5, so the GPU tests' 1e-4 is never strained by the reference arithmetic; and the recipe every other Renderer
test draws from reaches none of it, which is why the regimes exist."""
import pytest
import torch

import lightplane_amd as lp
from oracle import lightplane_oracle as O
from tests import partial_grad_cases as T
from tests import points_cases as PC
from tests import value_regime_cases as V
from tests.synth import RENDERER_CASES

ORACLE_TOL = 2e-5   # tests/test_oracle_golden.py REL_TOL: what the oracle itself is held to
F64 = torch.float64


def _err(a32, a64):
    return float((a32.double() - a64).abs().max()) / max(float(a64.abs().max()), 1e-30)


def _precondition(tag, d):
    """fp32 oracle vs fp64 oracle on the three outputs (tests/test_ragged_widths_host.py); finite everywhere"""
    o64, o32 = V.oracle_forward(d, F64), V.oracle_forward(d, torch.float32)
    for nm, a, b in zip(("ray_length", "neg_log_t", "feature"), o32, o64):
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), f"{tag} {nm}: the oracle is not finite"
        assert float(b.abs().max()) > 0, f"{tag} {nm}: zero everywhere"
        e = _err(a, b)
        print(f"{tag} {nm}: fp32 oracle vs fp64 oracle {e:.3e}")
        assert e <= ORACLE_TOL, f"{tag} {nm}: the fp32 and the fp64 oracle differ by {e:.3e} of the largest entry (bar {ORACLE_TOL:g})"


def _gradient_spread(tag, d):
    """fp32 oracle's gradients against the fp64 oracle's: printed (a ReLU tie of the fp32 oracle shows here; the GPU bar is against fp64)"""
    g32, g64 = V.oracle_gradients(d, torch.float32), V.oracle_gradients(d, F64)
    named = [("grad_mlp_params", g32[1], g64[1]), ("grad_encoding", g32[2], g64[2])] + \
        [(f"grad_grid{i}", a, b) for i, (a, b) in enumerate(zip(g32[3], g64[3]))] + \
        [(f"grad_color_grid{i}", a, b) for i, (a, b) in enumerate(zip(g32[4] or [], g64[4] or []))]
    worst = {nm: _err(a, b) for nm, a, b in named}
    print(f"{tag}: fp32 oracle's gradients vs fp64: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for nm, a, b in named:
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), f"{tag} {nm}: the oracle's gradient is not finite"
    return worst


# ---- the tables ---------------------------------------------------------------------------------------------------------------------------
def test_the_tables_hold_what_they_promise():
    assert [e.id for e in T.RENDERER_ENTRIES] == ["tuned_tri_c16", "tuned_vox_c32", "tuned_nonplain", "tuned_seg", "tuned_nw8", "tuned_tm",
                                                 "tuned_fp32", "loop_deep_424", "loop_shallow_h16", "loop_h64_two_block", "loop_c64", "loop_seg",
                                                 "loop_two_grid", "loop_two_grid_h64", "generic_lds", "generic_global", "flat_grid"]
    assert set(V.RENDERER_CONSTANTS) == set(V.RENDERER_PAIRS) and len(V.RENDERER_PAIRS) == 17 * 4
    assert set(V.DEEP_CONSTANTS) == set(V.DEEP_PAIRS) and len(V.DEEP_PAIRS) == 6
    assert len(V.POINTS_PAIRS) == 6 and {n for n, _ in V.POINTS_PAIRS} == {"triplane_c16_222x32", "voxel_c32_112x64_flat"}
    assert {r for _, r in V.POINTS_PAIRS} == set(V.POINT_REGIMES) and set(V.SCAFFOLD_CONSTANTS) == {"init", "extremes"}
    fams = [T.renderer_entry(i).family for i in V.ZERO_SPAN_ENTRIES]
    assert fams == [1, 3, 0]   # one tuned, one looped, one shape-generic
    assert set(V.LEDGER) == set(V.REGIMES)
    names = [p.__name__ for ps in V.LEDGER.values() for p in ps]
    assert len(set(names)) == len(names) == 14
    for ps in V.LEDGER.values():   # every predicate says which device lines it restates
        for p in ps:
            assert p.__doc__ and (".h:" in p.__doc__ or ".hip:" in p.__doc__), p.__name__
    for table in (V.POINTWISE, V.SCAFFOLD_POINTWISE):
        for regime, ps in table.items():
            assert set(ps) <= set(V.LEDGER[regime])
    for (i, regime), k in V.RENDERER_CONSTANTS.items():
        # three checkpoint blocks where the march is not segmented; segmented entries keep their 21 samples
        want = None if regime != "opaque_late" or T.renderer_entry(i).segmented else 70
        assert k.num_samples == want, (i, regime)


def test_the_transform_is_the_affine_map_and_touches_nothing_else():
    """On the entry with noise: raw_o' = a_o raw_o + b_o BEFORE the noise (the kernel adds the noise to the opacity head's output),
    raw_c' = a_c raw_c, the noise itself and every ReLU margin unchanged."""
    e = T.renderer_entry("tuned_nonplain")
    d = e.case.build()
    k = V.Constants(a_o=25.0, b_o=-10.0, a_c=40.0, gain=0.5)
    t = V.apply_regime(d, k)
    assert not torch.equal(t["decoder"].mlp_params, d["decoder"].mlp_params) and t["cfg"]["gain"] == 0.5
    assert t["cfg"]["inject_noise_sigma"] == 0.5 and t["rays"] is d["rays"] and t["grids"] is d["grids"]
    with O.relu_margin_recorder() as m0:
        _, r0 = V.oracle_forward(d, F64, record=True)
    with O.relu_margin_recorder() as m1:
        _, r1 = V.oracle_forward(t, F64, record=True)
    assert torch.equal(m0.margin, m1.margin)
    assert float((r1.raw_o - (25.0 * r0.raw_o - 10.0)).abs().max()) <= 1e-5 and float((r1.raw_c - 40.0 * r0.raw_c).abs().max()) <= 1e-5
    noise = r0.softplus_in - r0.raw_o
    assert float(noise.abs().max()) > 0.5 and float(((r1.softplus_in - r1.raw_o) - noise).abs().max()) <= 1e-12


# ---- what the suite reached before ----------------------------------------------------------------------------------------------------------
def test_the_recipe_of_the_other_tests_reaches_one_path_only():
    """DESIGN.md 2, "Value regimes", checked rather than remembered.  Over the unchanged RENDERER_CASES: no argument of the softplus is
    above 20 (linear branch) and no colour pre-activation saturates; -log T over the regular samples stays below 20 (T never reaches 0
    there; only the beyond-far samples, whose interval lengths grow to far / disparity_at_inf, take it to 1e5); and exactly ONE case --
    flex_121_h16_c32_noise, 24 rays -- has samples below -4.159 (series branch), down to -6.6.  Every other Renderer test runs the middle
    path of the compositing arithmetic."""
    hi, c_abs, top_regular, top, below = 0.0, 0.0, 0.0, 0.0, {}
    for c in RENDERER_CASES:
        _, r = V.oracle_forward(c.build(), F64, record=True)
        hi = max(hi, float(r.softplus_in.max()))
        c_abs = max(c_abs, float(r.raw_c.abs().max()))
        top_regular, top = max(top_regular, float(r.nlt[:, c.num_samples].max())), max(top, float(r.final.max()))
        n = int((r.softplus_in < V.SERIES_BELOW).sum())
        if n:
            below[c.name] = (n, r.softplus_in.numel(), float(r.softplus_in.min()))
    print(f"RENDERER_CASES: softplus argument <= {hi:.3g}, |raw_c| <= {c_abs:.3g}, -log T <= {top_regular:.3g} over the regular samples, "
          f"<= {top:.3g} with the beyond-far ones; below {V.SERIES_BELOW}: {below}")
    assert hi < V.OLD_COVERAGE["softplus_in_max"] and c_abs < V.OLD_COVERAGE["raw_c_abs_max"]
    assert top_regular < V.OLD_COVERAGE["regular_nlt_max"] < V.T_IS_ZERO
    assert set(below) == set(V.OLD_COVERAGE["series_branch_cases"]), below
    assert all(lo > V.OLD_COVERAGE["softplus_in_min"] for _, _, lo in below.values())


# ---- Renderer carriers ------------------------------------------------------------------------------------------------------------------------
def _selection_holds(e, d, forward_family=None):
    sel = T.renderer_selection(e, d)
    assert (sel["family"], sel["segments"]) == (e.family, e.segments), (e.id, sel)
    base = T.renderer_entry(e.id) if forward_family is None else e
    assert (e.family, e.segments, e.kernel, e.march_order, e.flat, e.config) == \
        (base.family, base.segments, base.kernel, base.march_order, base.flat, base.config)
    if e.march_order == "samples":
        assert sel["march"] == "samples"
    if forward_family is not None:
        with T.config_set(**e.config):
            got = lp.forward_kernel_family(d["rays"], d["grids"], d["decoder"], color_grid=d["color_grids"], num_samples_inf=d["cfg"]["num_samples_inf"])
        assert got == forward_family, (e.id, got)


@pytest.mark.parametrize("entry_id,regime", V.RENDERER_PAIRS + V.DEEP_PAIRS, ids=[f"{i}-{r}" for i, r in V.RENDERER_PAIRS + V.DEEP_PAIRS])
def test_renderer_pair_reaches_its_regime(entry_id, regime):
    deep = entry_id in V.DEEP_FORWARD_FAMILY
    e, d = V.built_deep(entry_id, regime) if deep else V.built_renderer(entry_id, regime)
    tag = f"{entry_id} [{regime}]"
    _selection_holds(e, d, V.DEEP_FORWARD_FAMILY.get(entry_id))
    own = e.case.build()
    assert not torch.equal(d["decoder"].mlp_params, own["decoder"].mlp_params), f"{tag}: the flat parameter tensor did not change"
    assert (d["scaffold"] is None) == (own["scaffold"] is None) and d["cfg"]["inject_noise_sigma"] == e.case.noise_sigma
    assert all(torch.equal(a, b) for a, b in zip(d["grids"], own["grids"])) and torch.equal(d["rays"].far, own["rays"].far)
    _, r = V.recorded_renderer(e, d)
    print(f"{tag}: {V.RENDERER_CONSTANTS.get((entry_id, regime)) or V.DEEP_CONSTANTS[(entry_id, regime)]} reaches {V.ranges(r)}")
    missed = V.missed(regime, r)
    assert not missed, f"{tag}: the fp64 oracle does not reach {missed}: {V.ranges(r)}"
    _precondition(tag, d)
    worst = max(_gradient_spread(tag, d).values())
    if (entry_id, regime) in V.CANCELLATION_PAIRS:   # w = T_{i-1} - T_i cancels in the reference's own formula: named, not reseeded away
        assert regime == "init" and ORACLE_TOL < worst <= 1e-4, f"{tag}: {worst:.3e}"
    else:
        assert worst <= ORACLE_TOL, f"{tag}: the fp32 oracle's gradients differ from the fp64 oracle's by {worst:.3e} (bar {ORACLE_TOL:g})"


@pytest.mark.parametrize("entry_id", V.ZERO_SPAN_ENTRIES)
def test_zero_span_rays_give_zeros_in_the_oracle(entry_id):
    """far == near on every fourth ray: w = 0 on every sample, so zero outputs and no contribution to any gradient (the encoding's rows of
    those rays are exactly 0; -log T's own gradient is g_nlt * delta = g_nlt * 0)."""
    e, d = V.built_renderer(entry_id, "zero_span")
    _selection_holds(e, d)
    flat = d["rays"].far == d["rays"].near
    assert int(flat.sum()) == (T.N_RAYS + 3) // 4 and bool(flat[::4].all())
    for dt in (torch.float32, F64):
        out, _, ge, _, _ = V.oracle_gradients(d, dt)
        for o in out:
            assert float(o[flat].abs().max()) == 0.0 and float(o[~flat].abs().max()) > 0.0
        assert float(ge[flat].abs().max()) == 0.0 and float(ge[~flat].abs().max()) > 0.0
    _precondition(f"{entry_id} [zero_span]", d)


# ---- points and the scaffold's lattice --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,regime", V.POINTS_PAIRS, ids=[f"{n}-{r}" for n, r in V.POINTS_PAIRS])
def test_points_pair_reaches_its_regime(name, regime):
    c, own = V.points_case(name, regime), PC.case(name)
    tag = f"points {name} [{regime}]"
    assert not torch.equal(c["dec"].mlp_params, own["dec"].mlp_params) and torch.equal(c["pts"], own["pts"])
    assert torch.equal(c["zeroed"], own["zeroed"]) and torch.equal(c["left_out"], own["left_out"])  # (no ReLU input moved)
    r = V.Recorded(c["raw_o"], c["raw_o"], c["raw_c"], None)
    print(f"{tag}: {V.POINTS_CONSTANTS[(name, regime)]} reaches {V.ranges(r)}")
    missed = V.missed(regime, r, V.POINTWISE)
    assert not missed, f"{tag}: the fp64 oracle does not reach {missed}: {V.ranges(r)}"
    with torch.no_grad():
        op32, col32 = O.eval_decoder(c["pts"], c["grids"], c["gidx"], c["dec"], c["enc"], PC.GAIN, mask_out_of_bounds_samples=c["mask"],
                                     scaffold=c["scaffold"], color_grids=c["cgrids"], contract_coords=c["contract"])
    keep = ~c["left_out"]
    for nm, a, b in (("opacity", op32[keep], c["op"][keep]), ("colour", col32[..., :3][keep], c["col"][keep])):
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
        print(f"{tag} {nm}: fp32 oracle vs fp64 oracle {_err(a, b):.3e}")
        assert _err(a, b) <= ORACLE_TOL, f"{tag} {nm}: {_err(a, b):.3e}"
    for g in [c["grads"]["params"], c["grads"]["enc"], c["grads"]["points"]] + c["grads"]["grids"]:
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0


@pytest.mark.parametrize("regime", list(V.SCAFFOLD_CONSTANTS))
def test_scaffold_lattice_reaches_its_regime(regime):
    c = V.scaffold_case(regime)
    missed = V.missed(regime, c["seen"], V.SCAFFOLD_POINTWISE)
    print(f"scaffold [{regime}]: {V.SCAFFOLD_CONSTANTS[regime]} reaches raw_o in {V.ranges(c['seen'])['raw_o']}, opacity <= {float(c['op'].max()):.4g}")
    assert not missed, f"scaffold [{regime}]: the fp64 oracle does not reach {missed}"
    assert c["seen"].raw_o.numel() == c["op"].numel() and bool(torch.isfinite(c["op"]).all()) and float(c["op"].max()) > 0
    if regime == "init":   # the oracle's gain * softplus, restated: every lattice point on the series branch
        want = c["gain"] * torch.log1p(torch.exp(c["seen"].raw_o))
        assert float((c["op"].flatten() - want.flatten()).abs().max()) <= 1e-15

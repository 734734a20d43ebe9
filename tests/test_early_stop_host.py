"""Early ray termination without a GPU: the truncated fp64 oracle (``last_sample``), the march rule (``oracle.early_stop_index``), the
table of scripted batches (tests/early_stop_cases.py: what it covers by the oracle's own count, and the tie condition that lets the GPU
test demand equal stop indices) and the dispatch under a stop through the entry points that need no GPU."""
import copy
import math

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib
from oracle import lightplane_oracle as O
from tests import early_stop_cases as E
from tests.synth import RendererCase
from tests.value_regime_cases import rays_as

F64 = torch.float64


def _tiny():
    d = RendererCase("tiny_stop", seed=77, n_rays=6, grid_base=(2, 4, 5, 3, 16), num_samples=7, num_samples_inf=2, gain=3.0).build()
    last = torch.tensor([8, 0, 3, 6, 7, 2])
    return d, last


def _oracle64(d, last, grad=True):
    rays = rays_as(d["rays"], F64)
    rays.encoding = rays.encoding.clone().requires_grad_(grad)
    dec = copy.copy(d["decoder"])
    dec.mlp_params = dec.mlp_params.to(F64).clone().requires_grad_(grad)
    grids = [g.to(F64).clone().requires_grad_(grad) for g in d["grids"]]
    out = O.lightplane_renderer_naive(rays, grids, dec, last_sample=last, **d["cfg"])
    if not grad:
        return out
    u = [x.to(F64) for x in d["upstream"]]
    ((out[0] * u[0]).sum() + (out[1] * u[1]).sum() + (out[2] * u[2]).sum()).backward()
    return out, dec.mlp_params.grad, rays.encoding.grad, [g.grad for g in grids]


def test_masked_oracle_equals_a_per_sample_loop():
    """The truncated march, written out: ray by ray, sample by sample, in Python floats, from the oracle's own per-sample opacity, colour,
    depth and interval length -- stopping behind ``last_sample[r]``."""
    d, last = _tiny()
    cfg = d["cfg"]
    S, S_inf = cfg["num_samples"], cfg["num_samples_inf"]
    rays = rays_as(d["rays"], F64)
    dec = copy.copy(d["decoder"])
    dec.mlp_params = dec.mlp_params.to(F64)
    grids = [g.to(F64) for g in d["grids"]]
    with torch.no_grad():
        got = O.lightplane_renderer_naive(rays, grids, dec, last_sample=last, **cfg)
        depths = O.ray_depths(rays.near, rays.far, S, S_inf, 1e-5)
        delta = O.ray_deltas(rays.near, rays.far, depths, S)
        points = depths[..., None] * rays.directions[:, None] + rays.origins[:, None]
        opacity, colour = O.eval_decoder(points, grids, rays.grid_idx, dec, rays.encoding, cfg["gain"])
    cc = int(dec.color_chn)
    for r in range(rays.n_rays):
        nlt, t_prev, length, feat = 0.0, 1.0, 0.0, [0.0] * cc
        for s in range(S + S_inf):
            if s > int(last[r]):
                break
            nlt += float(opacity[r, s]) * float(delta[r, s])
            t = math.exp(-nlt)
            w = t_prev - t
            t_prev = t
            length += w * float(depths[r, s])
            for c in range(cc):
                feat[c] += w * float(colour[r, s, c])
        assert abs(float(got[0][r]) - length) <= 1e-12 * max(1.0, abs(length)), r
        assert abs(float(got[1][r]) - nlt) <= 1e-12 * max(1.0, nlt), r
        for c in range(cc):
            assert abs(float(got[2][r, c]) - feat[c]) <= 1e-12, (r, c)


def test_masked_samples_get_exactly_zero_gradient():
    """Grid rows that only masked samples touch: gradient exactly 0 -- and they would have had one in the full march."""
    d, last = _tiny()
    cfg = d["cfg"]
    _, _, _, gg = _oracle64(d, last)
    _, _, _, gg_full = _oracle64(d, None)
    rows = O.renderer_corner_indices(d["rays"], d["sizes"], cfg["num_samples"], cfg["num_samples_inf"], cfg["contract_coords"])
    s = torch.arange(cfg["num_samples"] + cfg["num_samples_inf"])[None, :]
    live = s <= last[:, None]
    for g, g_full, rr in zip(gg, gg_full, rows):
        n_rows = g.numel() // g.shape[-1]
        touched_live = torch.zeros(n_rows, dtype=torch.bool)
        touched_masked = torch.zeros(n_rows, dtype=torch.bool)
        for m, sel in ((touched_live, live), (touched_masked, ~live)):
            hit = rr[sel].reshape(-1)
            m[hit[hit >= 0]] = True
        only_masked = touched_masked & ~touched_live
        assert int(only_masked.sum()) > 0, "the tiny case masks no sample with rows of its own"
        flat, flat_full = g.reshape(n_rows, -1), g_full.reshape(n_rows, -1)
        assert bool((flat[only_masked] == 0).all()), "a masked sample passed a gradient on"
        assert bool((flat_full[only_masked] != 0).any()), "those rows carry no gradient in the full march either: the check is empty"
    # and the truncated -log T is the running sum at the last contributing sample
    nlt_cum = E.neg_log_t_cum(d)
    out = _oracle64(d, last, grad=False)
    assert torch.allclose(out[1].detach(), nlt_cum.gather(1, last[:, None])[:, 0], rtol=1e-13, atol=0)


def test_full_length_last_sample_is_bit_identical_to_none():
    d, _ = _tiny()
    s_tot = d["cfg"]["num_samples"] + d["cfg"]["num_samples_inf"]
    a = _oracle64(d, None)
    b = _oracle64(d, torch.full((d["rays"].n_rays,), s_tot - 1, dtype=torch.int64))
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for x, y in zip(a[3], b[3]):
        assert torch.equal(x, y)
    # fp32 as well: the parity tests run the oracle in both
    d32 = dict(d)
    o_none = O.lightplane_renderer_naive(d["rays"], d["grids"], d["decoder"], **d["cfg"])
    o_full = O.lightplane_renderer_naive(d32["rays"], d["grids"], d["decoder"], last_sample=torch.full((d["rays"].n_rays,), s_tot - 1), **d["cfg"])
    assert all(torch.equal(x, y) for x, y in zip(o_none, o_full))


def test_early_stop_index_against_a_scripted_ledger():
    """Seven rays in groups of three (the last group holds one ray), five samples, threshold 4."""
    nlt = torch.tensor([
        # group 0: the middle ray holds it back until sample 3; reaching the threshold EXACTLY counts (the kernels vote ``nlt < stop``)
        [5.0, 6.0, 7.0, 8.0, 9.0],
        [0.5, 1.0, 3.5, 4.0, 4.5],
        [4.5, 9.0, 9.5, 50., 90.],
        # group 1: never stops -- one ray stays transparent
        [9.0, 9.0, 9.0, 9.0, 9.0],
        [0.0, 0.0, 0.0, 0.0, 0.0],
        [1.0, 2.0, 3.0, 3.5, 3.9],
        # group 2, part-filled: stops at sample 0 on its own ray alone
        [4.25, 5.0, 6.0, 7.0, 8.0],
    ], dtype=F64)
    st = O.early_stop_index(nlt, 4.0, 3)
    assert st.index.tolist() == [3, 4, 0]
    assert st.margin_reached.tolist() == [0.0, math.inf, 0.25]
    assert st.margin_before.tolist() == [0.5, 4.0, math.inf]
    # a group that reaches the threshold only at the last sample: the march ends there anyway, only the sample before decides
    st = O.early_stop_index(nlt[5:6] + torch.tensor([0, 0, 0, 0, 0.2], dtype=F64), 4.0, 3)
    assert st.index.tolist() == [4] and st.margin_reached.tolist() == [math.inf] and float(st.margin_before[0]) == 0.5
    # groups of one: every ray on its own
    assert O.early_stop_index(nlt, 4.0, 1).index.tolist() == [0, 3, 0, 0, 4, 4, 0]
    # a group larger than the batch
    assert O.early_stop_index(nlt, 4.0, 64).index.tolist() == [4]


@pytest.fixture(scope="module")
def built():
    return {c.name: E.build(c) for c in E.CASES}


def test_the_table_covers_what_it_claims(built):
    """By the oracle's own count, not by the scripts' intent."""
    seen = set()
    for c in E.CASES:
        d = built[c.name]
        idx = d["expected"].index.tolist()
        nlt, thr = d["neg_log_t_full"], c.stop_neg_log_t
        assert len(idx) == len(c.groups) == -(-c.n_rays // c.group), c.name
        assert [g.target if g.target is not None else c.s_tot - 1 for g in c.groups] == idx, f"{c.name}: the oracle's indices {idx} are not the scripted ones"
        never = [bool(nlt[g * c.group:(g + 1) * c.group, -1].min() < thr) for g in range(len(idx))]
        if 0 in idx:
            seen.add("stop at sample 0")
        if 31 in idx and 32 in idx:
            seen.add("stops at 31 and at 32: either side of a -log T checkpoint")
        per_wg = c.workgroup // c.group
        for w in range(0, len(idx), per_wg):
            stopping = {i for i, nv in zip(idx[w:w + per_wg], never[w:w + per_wg]) if not nv}
            if any(never[w:w + per_wg]) and len(stopping) >= 3:
                seen.add("a group that never stops beside groups that stop at three or more samples, in one workgroup")
        if c.n_rays % c.group and not never[-1] and idx[-1] < c.s_tot - 1:
            seen.add(f"a part-filled last group of {c.group} that stops")
        if any(E.S <= i < c.s_tot - 1 for i in idx):
            seen.add("a stop inside the beyond-far samples")
        if c.noise_sigma > 0 and c.contract and c.mask_oob:
            seen.add("noise + contraction + out-of-bounds mask")
        if c.pool and d["scaffold"] is not None and any(float(nlt[g * c.group:(g + 1) * c.group, -1].min()) == 0.0 for g in range(len(idx))):
            seen.add("rays through the empty half-space of a scaffold")
        for g, spec in enumerate(c.groups):
            if spec.held:
                grp = nlt[g * c.group:(g + 1) * c.group, idx[g]]
                slow = grp < thr + 0.5 * thr
                if int(slow.sum()) == spec.held and float(grp[~slow].min()) > 80.0:
                    seen.add("a group held back by a single transparent ray, the others beyond -log T = 80")
        fam = 0 if c.kernel == _lib.LP_KERNEL_GENERIC else lp.kernel_family(d["rays"], d["grids"], d["decoder"], color_grid=d["color_grids"],
                                                                            num_samples_inf=c.num_samples_inf)
        assert fam == c.family, f"{c.name}: kernel family {fam}, the table says {c.family}"
        C = int(d["grids"][0].shape[-1])
        seen.add({0: "shape-generic", 1: f"tuned C = {C}", 3: "layer-looped"}[fam])
        if fam == 3:
            seen.add(f"layer-looped {'two-grid' if c.separate_color_grid else '/'.join(map(str, c.n_layers)) + ' x ' + str(c.hidden)}")
    want = {"stop at sample 0", "stops at 31 and at 32: either side of a -log T checkpoint",
            "a group that never stops beside groups that stop at three or more samples, in one workgroup",
            "a part-filled last group of 32 that stops", "a part-filled last group of 64 that stops", "a stop inside the beyond-far samples",
            "noise + contraction + out-of-bounds mask", "rays through the empty half-space of a scaffold",
            "a group held back by a single transparent ray, the others beyond -log T = 80",
            "shape-generic", "tuned C = 16", "tuned C = 32", "layer-looped", "layer-looped two-grid", "layer-looped 1/1/2 x 64",
            "layer-looped 3/3/3 x 32"}
    assert want <= seen, f"not covered: {sorted(want - seen)}"


@pytest.mark.parametrize("case", E.CASES, ids=E.CASE_IDS)
def test_tie_condition(case, built):
    """Both decisive margins of every group clear 10 x (1e-4 x the largest -log T the truncated march returns): a kernel that meets the
    suite's bar on -log T cannot take another index than the oracle's."""
    d = built[case.name]
    st = d["expected"]
    assert d["tie_bar"] == 10.0 * 1e-4 * d["max_neg_log_t"] and d["max_neg_log_t"] >= case.stop_neg_log_t
    for g in range(len(st.index)):
        assert float(st.margin_reached[g]) >= d["tie_bar"] and float(st.margin_before[g]) >= d["tie_bar"], (
            f"{case.name} group {g} (stops at {int(st.index[g])}): margins {float(st.margin_reached[g]):.4f} / {float(st.margin_before[g]):.4f} "
            f"under the bar {d['tie_bar']:.4f}")
    # the truncated oracle agrees with the full march up to every ray's last sample, and returns -log T there
    nlt_t = E.neg_log_t_cum(d, d["last_sample"])
    full = d["neg_log_t_full"]
    s = torch.arange(case.s_tot)[None, :]
    live = s <= d["last_sample"][:, None]
    assert torch.equal(nlt_t[live], full[live])
    assert torch.equal(nlt_t[:, -1], full.gather(1, d["last_sample"][:, None])[:, 0])
    flags = E.expected_flags(case, d["last_sample"])
    assert flags.shape == (case.n_rays, case.s_tot) and bool(((flags == 1) == live).all())
    if case.workgroup == case.group:
        assert not bool((flags == 2).any())       # one wave per workgroup: nobody to wait for
    else:
        assert bool((flags == 2).any()) and bool((flags == 0).any())


def test_dispatch_under_a_stop():
    """What the library decides about a launch with early termination, through the queries that need no GPU: a small batch is not split
    into ray segments (a segment would need the stop of the segments before it), and it does not march samples per wavefront either
    (``renderer_tm_eligible``: a wave would hold one ray -- no vote); without the stop both answers differ."""
    d = E.build(E.CASES[0])
    args = (d["rays"], d["grids"], d["decoder"], E.S)
    n_seg = -(-E.S // 8)
    assert lp.renderer.backward_segments(*args) == n_seg                                         # small batch, rays per wave: segmented
    assert lp.renderer.backward_segments(*args, march_order="samples") == 1                       # the transposed march never segments
    for order in ("rays", "samples"):
        assert lp.renderer.backward_segments(*args, stop_transmittance=d["stop_transmittance"], march_order=order) == 1
    # the stop is what the ABI carries as -log: the Python front end and the oracle's threshold are the same number
    assert E.CASES[0].stop_neg_log_t == -math.log(d["stop_transmittance"])

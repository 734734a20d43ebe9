"""GPU tests of the ray clip (lp.clip_rays_to_scaffold / lp_rays_clip, csrc/lp_ray_clip.hip) against the fp64 brute-force oracle and the
checks of tests/ray_clip_cases.py (its docstring states the cases, the ambiguity rule and its cap, and the derived tolerance).  The
kernel runs once per (case, pad); every test reads those results and leaves them unchanged.  Figures are printed before they are asserted."""
import importlib.util
import math
import os

import pytest
import torch

import lightplane_amd as lp
from tests import ray_clip_cases as RC
from tests.synth import grid_sizes_for, random_decoder, random_grids
from tests.test_gpu_parity import _dev

pytestmark = pytest.mark.gpu

_RESULTS = {}


def _rays_on(c, dev):
    return lp.Rays(directions=c["d"].to(dev), origins=c["o"].to(dev), grid_idx=c["grid_idx"].to(dev), near=c["near"].to(dev),
                   far=c["far"].to(dev), encoding=None)


def _case(name):
    return RC.glider_case(name) if name in RC.GLIDER_NAMES else RC.case(name)


def _clip(name, pad):
    """(near', far', hit) on the CPU for case `name` at `pad`: one kernel launch per pair, shared by the tests"""
    if (name, pad) not in _RESULTS:
        dev = _dev()
        c = _case(name)
        sc = None if c["scaffold"] is None else c["scaffold"].to(dev)
        clipped, hit = lp.clip_rays_to_scaffold(_rays_on(c, dev), sc, pad=pad)
        assert hit.dtype == torch.bool and hit.shape == (len(c["kind"]),)
        _RESULTS[(name, pad)] = (clipped.near.cpu(), clipped.far.cpu(), hit.cpu())
    return _RESULTS[(name, pad)]


@pytest.mark.parametrize("pad", RC.PADS)
@pytest.mark.parametrize("name", RC.CASE_NAMES + RC.GLIDER_NAMES)
def test_conservative(name, pad):
    """every ray, the ambiguous and ill-conditioned ones included: no sample of the Renderer's schedules K = 2048, 7, 64, 128 with a
    non-zero scaffold value lies outside [near', far'] of a hit ray or on a missed ray; near <= near' <= far' <= far.  Also on the face
    gliders of tests/ray_clip_cases.py: rays along a cell face within rounding whose span ends or begins inside the box."""
    c = _case(name)
    near_o, far_o, hit = _clip(name, pad)
    print(f"{name} pad {pad}: {int(hit.sum())} of {len(c['kind'])} rays hit")
    RC.check_conservative(c, near_o, far_o, hit, ks=(2048, 7, 64, 128))


@pytest.mark.parametrize("pad", RC.PADS)
@pytest.mark.parametrize("name", RC.CASE_NAMES + RC.GLIDER_NAMES)
def test_exact_misses(name, pad):
    c = _case(name)
    RC.check_misses(c, *_clip(name, pad))


@pytest.mark.parametrize("pad", RC.PADS)
@pytest.mark.parametrize("name", RC.CASE_NAMES)
def test_tight(name, pad):
    """unambiguous, well-conditioned rays: hit == hit64 and expected - 2 tol <= near' <= expected + tol (mirrored for far') with
    tol = 16 * 2^-24 * max_a (1 + |o_a|) / |d_a| + 4 * 2^-24 * |t|"""
    c = RC.case(name)
    n, worst = RC.check_tight(c, *_clip(name, pad), pad)
    print(f"{name} pad {pad}: {n} rays compared, the loosest end uses {worst:.3f} of its tolerance (2 allowed outwards)")


def test_special_scaffolds():
    dev = _dev()
    # no scaffold: the box's slab interval (the "box" case's oracle is one occupied cell [-1, 1]^3; test_tight holds its ends)
    cb = RC.case("box")
    m = RC.tight_mask(cb)
    assert torch.equal(_clip("box", 0.0)[2][m], cb["oracle"]["hit"][m]) and int(cb["oracle"]["hit"][m].sum()) > 100
    # all ones: what no scaffold gives on the same rays, up to the roundings of a crossing on either side (pad 0: h differs)
    co = RC.case("ones_8")
    near_o, far_o, hit_o = _clip("ones_8", 0.0)
    clipped, hit_n = lp.clip_rays_to_scaffold(_rays_on(co, dev), None, pad=0.0)
    near_n, far_n, hit_n = clipped.near.cpu(), clipped.far.cpu(), hit_n.cpu()
    m = RC.tight_mask(co) & torch.tensor([k != "grid_idx_out_of_range" for k in co["kind"]])  # (without a scaffold every index >= 0 is the box)
    assert torch.equal(hit_n[m], hit_o[m])
    m = m & hit_o
    assert int(m.sum()) > 100
    q = torch.where(co["d"] != 0, (1.0 + co["o"].abs()) / co["d"].abs(), torch.zeros(())).max(dim=1).values.double()
    assert bool(((near_n.double() - near_o.double()).abs()[m] <= 32 * RC.U * q[m]).all())
    assert bool(((far_n.double() - far_o.double()).abs()[m] <= 32 * RC.U * q[m]).all())
    # all zeros / an empty single cell: all misses
    for name in ("zeros_8", "one_cell_empty"):
        for pad in RC.PADS:
            assert not bool(_clip(name, pad)[2].any()), (name, pad)
    # a single full cell: hit exactly where the box alone is hit
    assert torch.equal(_clip("one_cell_full", 0.0)[2][RC.tight_mask(cb)], RC.case("one_cell_full")["oracle"]["hit"][RC.tight_mask(cb)])
    # batch: scene 1's rays do not see scene 0's cells
    c = RC.case("random_2x5x6x7")
    sc = c["scaffold"].clone()
    base = _clip("random_2x5x6x7", 0.5)
    sc[0] = 1.0 - (sc[0] != 0).float()  # scene 0 inverted
    clipped, hit = lp.clip_rays_to_scaffold(_rays_on(c, dev), sc.to(dev), pad=0.5)
    one = c["grid_idx"] == 1
    assert int(one.sum()) > 50
    assert torch.equal(clipped.near.cpu()[one], base[0][one]) and torch.equal(clipped.far.cpu()[one], base[1][one])
    assert torch.equal(hit.cpu()[one], base[2][one])
    zero = c["grid_idx"] == 0
    assert not torch.equal(hit.cpu()[zero], base[2][zero])


def test_aliasing_reproducibility_and_graph_capture():
    dev = _dev()
    c = RC.case("shell_16")
    sc = c["scaffold"].to(dev)
    want = _clip("shell_16", 0.5)
    rays = _rays_on(c, dev)
    # shares what it does not change
    clipped, hit = lp.clip_rays_to_scaffold(rays, sc, pad=0.5)
    assert clipped.directions is rays.directions and clipped.origins is rays.origins and clipped.grid_idx is rays.grid_idx
    assert clipped.near is not rays.near and clipped.far is not rays.far
    for got, ref in zip((clipped.near, clipped.far), want[:2]):  # two launches: bit-identical (NaN entries compare as bits)
        assert torch.equal(got.cpu().view(torch.int32), ref.view(torch.int32))
    assert torch.equal(hit.cpu(), want[2])
    # in place: the results alias the inputs
    near, far, hit8 = rays.near.clone(), rays.far.clone(), torch.empty(RC.R, dtype=torch.uint8, device=dev)
    inplace = lp.Rays(directions=rays.directions, origins=rays.origins, grid_idx=rays.grid_idx, near=near, far=far, encoding=None)
    clipped, hit = lp.clip_rays_to_scaffold(inplace, sc, pad=0.5, out=(near, far, hit8))
    assert clipped.near is near and clipped.far is far
    assert torch.equal(near.cpu().view(torch.int32), want[0].view(torch.int32)) and torch.equal(far.cpu().view(torch.int32), want[1].view(torch.int32))
    assert torch.equal(hit8.bool().cpu(), want[2])
    # one launch captured in a graph and replayed
    o_near, o_far, o_hit = torch.zeros_like(rays.near), torch.zeros_like(rays.far), torch.zeros(RC.R, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        lp.clip_rays_to_scaffold(rays, sc, pad=0.5, out=(o_near, o_far, o_hit))  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    for t in (o_near, o_far, o_hit):
        t.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lp.clip_rays_to_scaffold(rays, sc, pad=0.5, out=(o_near, o_far, o_hit))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(o_near.cpu().view(torch.int32), want[0].view(torch.int32)) and torch.equal(o_far.cpu().view(torch.int32), want[1].view(torch.int32))
    assert torch.equal(o_hit.bool().cpu(), want[2])


def test_tensors_on_another_device_are_refused():
    """every tensor has to live on the rays' GPU: _lib.check_tensors raises before a pointer reaches the library"""
    dev = _dev()
    c = RC.case("shell_16")
    rays = _rays_on(c, dev)
    with pytest.raises(AssertionError, match="scaffold is on cpu"):
        lp.clip_rays_to_scaffold(rays, c["scaffold"], pad=0.5)
    mixed = lp.Rays(directions=rays.directions, origins=rays.origins, grid_idx=rays.grid_idx, near=rays.near, far=rays.far, encoding=None)
    mixed.far = c["far"]  # (after the constructor's own device check)
    with pytest.raises(AssertionError, match="rays.far is on cpu"):
        lp.clip_rays_to_scaffold(mixed, c["scaffold"].to(dev), pad=0.5)
    out = (torch.empty(RC.R, device=dev), torch.empty(RC.R), torch.empty(RC.R, dtype=torch.uint8, device=dev))
    with pytest.raises(AssertionError, match=r"out\[1\] is on cpu"):
        lp.clip_rays_to_scaffold(rays, c["scaffold"].to(dev), pad=0.5, out=out)


def test_end_to_end_with_the_renderer():
    """a small default-shape triplane render (S = 32, the [2, 5, 6, 7] scaffold, 257 rays): missed rays have alpha == 0 exactly on the
    original rays; the clipped rays render and are finite.  (The Renderer refuses a grid_idx out of range and a NaN ray is no render: those
    six rays are replaced by the first one.)"""
    dev = _dev()
    c = RC.case("random_2x5x6x7")
    bad = torch.tensor([k in ("non_finite", "grid_idx_out_of_range") for k in c["kind"]])
    f = {k: torch.where(bad.reshape(-1, *([1] * (c[k].ndim - 1))), c[k][:1], c[k]) for k in ("o", "d", "near", "far", "grid_idx")}
    gen = torch.Generator().manual_seed(3)
    grids = [g.to(dev) for g in random_grids(gen, grid_sizes_for([2, 8, 8, 8, 16], True))]
    dec = random_decoder(gen, 2, 2, 2, 16, 32, 3, std=0.3)
    dec = lp.DecoderParams(dec.mlp_params.to(dev), dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
    rays = lp.Rays(directions=f["d"].to(dev), origins=f["o"].to(dev), grid_idx=f["grid_idx"].to(dev), near=f["near"].to(dev),
                   far=f["far"].to(dev), encoding=torch.randn(RC.R, 32, generator=gen).to(dev))
    sc = c["scaffold"].to(dev)
    clipped, hit = lp.clip_rays_to_scaffold(rays, sc, pad=0.5)
    assert clipped.encoding is rays.encoding
    _, nlt, _ = lp.lightplane_renderer(rays, grids, dec, num_samples=32, gain=1.0, scaffold=sc)
    alpha = 1.0 - torch.exp(-nlt)
    print(f"{int((~hit).sum())} of {RC.R} rays missed; alpha of the others {float(alpha[hit].min()):.3g} .. {float(alpha[hit].max()):.3g}")
    assert 0 < int((~hit).sum()) < RC.R
    assert bool((alpha[~hit] == 0).all()) and bool((nlt[~hit] == 0).all())
    assert float(alpha[hit].max()) > 0
    length, nlt_c, feat = lp.lightplane_renderer(clipped, grids, dec, num_samples=32, gain=1.0, scaffold=sc)
    for t in (length, nlt_c, feat):
        assert bool(torch.isfinite(t).all())
    assert bool((nlt_c[~hit] == 0).all())


def test_example_clips_rays():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("fit_synthetic_scene", os.path.join(repo, "examples", "fit_synthetic_scene.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    old = lp.config.stop_transmittance
    try:
        r = mod.main(["--steps", "60", "--rays", "2048", "--res", "16", "--scaffold-steps", "30", "--scaffold-size", "24",
                      "--scaffold-threshold", "0.05", "--clip-rays"])
    finally:
        lp.config.stop_transmittance = old
    print("fit with clipped rays:", r)
    assert math.isfinite(r["first_loss"]) and math.isfinite(r["last_loss"]) and math.isfinite(r["heldout_psnr_db"])
    assert 0 < r["mean_span_ratio"] < 1
    assert 0 < r["hit_fraction"] <= 1

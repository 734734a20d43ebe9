"""The fused gather / splat of a grid-list at points (lightplane_amd/point_grid.py, csrc/lp_point_grid.hip) against its fp64 definition.

Oracle, inputs, and the points left out / zeroed: tests/point_grid_cases.py (its docstring states every condition and cap;
tests/test_point_grid_host.py::test_inputs_are_admissible checks them without a GPU).  Every comparison is held to the project's bar,
max |err| / max |ref| <= 1e-4 per tensor, and prints its figure before it asserts.
"""
import itertools

import pytest
import torch

import lightplane_amd as lp
from oracle import lightplane_oracle as O
from tests import point_grid_cases as PG
from tests.synth import random_rays
from tests.test_gpu_parity import _dev

pytestmark = pytest.mark.gpu

ALL = list(PG.CASES)


def _worst(name, got, want, keep=None):
    """max |err| / max |ref| over the kept entries, printed and held to the bar"""
    got, want = got.detach().double().cpu(), want.double().cpu()
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    if keep is not None:
        k = keep.reshape(keep.shape + (1,) * (want.ndim - keep.ndim)).expand_as(want)
        got, want = got[k], want[k]
    scale = max(float(want.abs().max()), 1e-30)
    err = float((got - want).abs().max()) / scale
    print(f"{name}: max |err| / max |ref| = {err:.3e} (max |ref| {scale:.4g})")
    assert err <= PG.TOL, f"{name}: {err:.3e} > {PG.TOL}"


def _as_list(g):
    return g if isinstance(g, list) else [g]


def _gather(c, grid, sizes, pts, gidx=None):
    return lp.sample_grid_at_points(pts, grid, c["gidx"].to(pts.device) if gidx is None else gidx, c["mask"], c["contract"],
                                    grid_sizes=sizes)


def _splat(c, pts, feat, normalize, gidx=None, sizes=None, as_list=None):
    as_list = c["form"] == "list" if as_list is None else as_list
    out = lp.splat_points(pts, feat, c["sizes"] if sizes is None else sizes, c["gidx"].to(pts.device) if gidx is None else gidx,
                          c["mask"], c["contract"], normalize=normalize, return_list=as_list)
    assert isinstance(out, list) == as_list
    return _as_list(out)


@pytest.mark.parametrize("name", ALL)
def test_gather_values(name):
    dev, c = _dev(), PG.case(name)
    grid, sizes = PG.grid_arg(c, c["grids"], dev)
    pts = c["pts"].to(dev)
    out = _gather(c, grid, sizes, pts)
    R, N = c["pts"].shape[:2]
    assert out.shape == (R, N, c["vec"].shape[-1]) and out.dtype == torch.float32 and out.device == dev
    _worst(f"{name} gather", out, c["gather"], ~c["left_out"])
    assert torch.equal(_gather(c, grid, sizes, pts), out), "a second call differs (the gather has no atomics)"
    other = dict(c, form="flat" if c["form"] == "list" else "list")
    grid2, sizes2 = PG.grid_arg(other, c["grids"], dev)
    assert torch.equal(_gather(c, grid2, sizes2, pts), out), "the list and the flat form of the same grids differ"


@pytest.mark.parametrize("name", ALL)
def test_gather_gradients(name):
    dev, c = _dev(), PG.case(name)
    n = c["zeroed"].numel()
    assert int(c["zeroed"].sum()) <= PG.MAX_ZEROED * n or n == 1 and not bool(c["zeroed"].any())
    grid, sizes = PG.grid_arg(c, c["grids"], dev, requires_grad=True)
    pts = c["pts"].to(dev).requires_grad_(True)
    out = _gather(c, grid, sizes, pts)
    d_grids = torch.autograd.grad(out, _as_list(grid), c["vec"].to(dev), retain_graph=True)
    for i, (got, want) in enumerate(zip(d_grids, PG.in_form(c, c["d_grid"]))):
        _worst(f"{name} gather: d grid[{i}]", got, want)
    (d_pts,) = torch.autograd.grad(out, pts, c["vec_live"].to(dev))
    _worst(f"{name} gather: d points", d_pts, c["d_points_gather"])


@pytest.mark.parametrize("name", ALL)
def test_splat_values(name):
    dev, c = _dev(), PG.case(name)
    pts, feat = c["pts"].to(dev), c["vec_kept"].to(dev)
    raw = _splat(c, pts, feat, False)
    norm = _splat(c, pts, feat, True)
    untouched = [w.reshape(-1) == 0 for w in PG.in_form(c, c["weights"])]
    for i, (got, want) in enumerate(zip(raw, PG.in_form(c, c["splat_raw"]))):
        _worst(f"{name} raw splat[{i}]", got, want)
    for i, (got, want) in enumerate(zip(norm, PG.in_form(c, c["splat_norm"]))):
        _worst(f"{name} normalised splat[{i}]", got, want)
    for got in (raw, norm):
        for g, u in zip(got, untouched):
            rows = g.reshape(u.numel(), -1).cpu()[u]
            assert rows.numel() == 0 or float(rows.abs().max()) == 0.0, "a row no point touches is not exactly 0"
    # the other return form holds the same numbers
    other = _splat(c, pts, feat, False, as_list=c["form"] != "list")
    flat = lambda gs: torch.cat([g.reshape(-1, g.shape[-1]) for g in gs])  # noqa: E731
    _worst(f"{name} raw splat, other return form", flat(other), flat(raw).cpu())


@pytest.mark.parametrize("name", ALL)
def test_splat_gradients(name):
    dev, c = _dev(), PG.case(name)
    ups = [u.to(dev) for u in PG.in_form(c, c["up_grids"])]
    keep = ~c["left_out"]
    for normalize, want in ((False, c["gather_up"]), (True, c["gather_up_norm"])):
        feat = c["vec"].to(dev).requires_grad_(True)
        outs = _splat(c, c["pts"].to(dev), feat, normalize)
        sum((o * u).sum() for o, u in zip(outs, ups)).backward()
        _worst(f"{name} splat (normalize={normalize}): d features", feat.grad, want, keep)
    pts = c["pts"].to(dev).requires_grad_(True)
    outs = _splat(c, pts, c["vec_live"].to(dev), False)
    sum((o * u).sum() for o, u in zip(outs, ups)).backward()
    _worst(f"{name} raw splat: d points", pts.grad, c["d_points_splat"])


@pytest.mark.parametrize("name", ALL)
def test_gather_and_splat_are_adjoint(name):
    """from GPU results alone, both sides summed in fp64: <gather(G, P), U> = <G, splat(P, U)>"""
    dev, c = _dev(), PG.case(name)
    grids = [g.to(dev) for g in c["grids"]]
    pts, vec = c["pts"].to(dev), c["vec_kept"].to(dev)
    gathered = lp.sample_grid_at_points(pts, grids, c["gidx"].to(dev), c["mask"], c["contract"])
    splatted = _splat(c, pts, vec, False, as_list=True)
    lhs = gathered.double() * vec.double()
    rhs = [g.double() * s.double() for g, s in zip(grids, splatted)]
    a, b = float(lhs.sum()), float(sum(r.sum() for r in rhs))
    scale = min(float(lhs.abs().sum()), float(sum(r.abs().sum() for r in rhs)))
    print(f"{name}: <gather, U> = {a:.9g}, <G, splat> = {b:.9g}, |difference| / sum |products| = {abs(a - b) / scale:.3e}")
    assert abs(a - b) <= PG.TOL * scale


def test_splat_of_the_splatters_points_is_the_splatter():
    """the Splatter's own sample points (fp32, 16 samples, 64 rays, no contraction) with the ray's encoding repeated per sample,
    normalised: lightplane_splatter on the same rays"""
    dev = _dev()
    gen = torch.Generator().manual_seed(41)
    sizes = [[2, 6, 5, 7, 16], [2, 1, 6, 7, 16]]
    rays = random_rays(gen, 64, 2, 16)
    pts = O._splatter_points(rays, 16, 0, False, 1e-5)
    assert pts.dtype == torch.float32 and pts.shape == (64, 16, 3)
    feat = rays.encoding[:, None, :].expand(-1, 16, -1).contiguous()
    want = lp.lightplane_splatter(rays.to(dev), sizes, num_samples=16)
    got = lp.splat_points(pts.to(dev), feat.to(dev), sizes, rays.grid_idx.to(dev), normalize=True)
    for i, (g, w) in enumerate(zip(got, want)):
        assert float(w.abs().max()) > 0
        _worst(f"splat_points vs lightplane_splatter, grid {i}", g, w)


def test_masked_points_add_nothing_and_get_nothing():
    """(the contraction maps every point into the box: the case with both has nothing to mask)"""
    name = "voxel_c5_mask"
    dev, c = _dev(), PG.case(name)
    inside = c["inside"]
    n_out = int((~inside).sum())
    assert 0 < n_out < inside.numel() and int(c["left_out"].sum()) == 0
    C = c["vec"].shape[-1]
    # one row per point, so that a subset of the points is a batch again
    pts = c["pts"].reshape(-1, 1, 3).to(dev)
    vec = c["vec"].reshape(-1, 1, C).to(dev)
    gidx = c["gidx"][:, None].expand(inside.shape).reshape(-1).to(dev)
    m = inside.reshape(-1).to(dev)
    for normalize in (False, True):
        outside_only = _splat(c, pts[~m], vec[~m], normalize, gidx=gidx[~m])
        assert all(float(g.abs().max()) == 0.0 for g in outside_only), "points outside the box added something"
        every = _splat(c, pts, vec, normalize, gidx=gidx)
        kept = _splat(c, pts[m], vec[m], normalize, gidx=gidx[m])
        for i, (a, b) in enumerate(zip(every, kept)):
            _worst(f"{name} normalize={normalize}: all points vs the points inside, grid {i}", a, b)
    # gather: exactly zero features, point gradient and (splat backward) feature gradient outside
    grids = [g.to(dev).requires_grad_(True) for g in c["grids"]]
    p = pts.clone().requires_grad_(True)
    out = lp.sample_grid_at_points(p, grids, gidx, True, c["contract"])
    assert float(out.detach()[~m].abs().max()) == 0.0 and float(out.detach()[m].abs().max()) > 0.0
    (out * vec).sum().backward()
    assert float(p.grad[~m].abs().max()) == 0.0 and float(p.grad[m].abs().max()) > 0.0
    f, p = vec.clone().requires_grad_(True), pts.clone().requires_grad_(True)
    outs = lp.splat_points(p, f, c["sizes"], gidx, True, c["contract"], normalize=False)
    sum((o * u.to(dev)).sum() for o, u in zip(outs, c["up_grids"])).backward()
    assert float(f.grad[~m].abs().max()) == 0.0 and float(f.grad[m].abs().max()) > 0.0
    assert float(p.grad[~m].abs().max()) == 0.0 and float(p.grad[m].abs().max()) > 0.0
    f = vec.clone().requires_grad_(True)
    outs = lp.splat_points(pts, f, c["sizes"], gidx, True, c["contract"], normalize=True)
    sum((o * u.to(dev)).sum() for o, u in zip(outs, c["up_grids"])).backward()
    assert float(f.grad[~m].abs().max()) == 0.0 and float(f.grad[m].abs().max()) > 0.0


def _subsets(names):
    return [s for k in range(1, len(names) + 1) for s in itertools.combinations(names, k)]


def test_gather_partial_gradients():
    dev, c = _dev(), PG.case("triplane_c16")
    vec = c["vec"].to(dev)

    def run(subset):
        grids = [g.to(dev).requires_grad_("grids" in subset) for g in c["grids"]]
        pts = c["pts"].to(dev).requires_grad_("points" in subset)
        out = _gather(c, grids, None, pts)
        (out * vec).sum().backward()
        return out.detach(), grids, pts

    ref_out, ref_grids, ref_pts = run(("grids", "points"))
    for subset in _subsets(("grids", "points")):
        out, grids, pts = run(subset)
        assert torch.equal(out, ref_out), subset
        if "points" in subset:
            assert torch.equal(pts.grad, ref_pts.grad), f"{subset}: the stored point gradient differs"
        else:
            assert pts.grad is None, f"{subset}: points did not ask and got a gradient"
        for i, (g, r) in enumerate(zip(grids, ref_grids)):
            if "grids" in subset:
                _worst(f"{subset}: d grid[{i}] vs all leaves", g.grad, r.grad)
            else:
                assert g.grad is None, f"{subset}: grid {i} did not ask and got a gradient"
    # one grid of the list alone
    grids = [g.to(dev).requires_grad_(i == 1) for i, g in enumerate(c["grids"])]
    (_gather(c, grids, None, c["pts"].to(dev)) * vec).sum().backward()
    assert grids[0].grad is None and grids[2].grad is None
    _worst("only grid 1 asks: d grid[1] vs all leaves", grids[1].grad, ref_grids[1].grad)


def test_raw_splat_partial_gradients():
    dev, c = _dev(), PG.case("triplane_c16")
    ups = [u.to(dev) for u in c["up_grids"]]

    def run(subset):
        feat = c["vec"].to(dev).requires_grad_("features" in subset)
        pts = c["pts"].to(dev).requires_grad_("points" in subset)
        outs = _splat(c, pts, feat, False)
        sum((o * u).sum() for o, u in zip(outs, ups)).backward()
        return [o.detach() for o in outs], feat, pts

    ref_outs, ref_feat, ref_pts = run(("features", "points"))
    for subset in _subsets(("features", "points")):
        outs, feat, pts = run(subset)
        for i, (o, r) in enumerate(zip(outs, ref_outs)):  # (summed with atomics: the order differs from call to call)
            _worst(f"{subset}: splat[{i}] vs all leaves", o, r)
        for key, t, r in (("features", feat, ref_feat), ("points", pts, ref_pts)):
            if key in subset:
                assert torch.equal(t.grad, r.grad), f"{subset}: the stored gradient of {key} differs"
            else:
                assert t.grad is None, f"{subset}: {key} did not ask and got a gradient"
    # only one of the returned grids is differentiated: the others count as zero upstream gradients
    feat = c["vec"].to(dev).requires_grad_(True)
    outs = _splat(c, c["pts"].to(dev), feat, False)
    (outs[1] * ups[1]).sum().backward()
    want = O.sample_grid_list([torch.zeros_like(u) if i != 1 else u.double() for i, u in enumerate(c["up_grids"])], c["pts"].double(),
                              c["gidx"], False)
    _worst("only splat[1] is differentiated: d features", feat.grad, want)


@pytest.mark.parametrize("shape", [(0, 5), (4, 0)])
def test_empty_batches(shape):
    dev, c = _dev(), PG.case("triplane_c16")
    grids = [g.to(dev).requires_grad_(True) for g in c["grids"]]
    pts = torch.zeros(*shape, 3, device=dev, requires_grad=True)
    idx = torch.zeros(shape[0], dtype=torch.long, device=dev)
    out = lp.sample_grid_at_points(pts, grids, idx)
    assert out.shape == shape + (16,)
    out.sum().backward()
    assert pts.grad.shape == pts.shape and all(float(g.grad.abs().max()) == 0.0 for g in grids)
    for normalize in (False, True):
        for as_list in (True, False):
            feat = torch.zeros(*shape, 16, device=dev, requires_grad=True)
            outs = lp.splat_points(pts.detach(), feat, c["sizes"], idx, normalize=normalize, return_list=as_list)
            if as_list:
                assert [list(o.shape) for o in outs] == c["sizes"]
            else:
                assert outs.shape == (sum(s[0] * s[1] * s[2] * s[3] for s in c["sizes"]), 16)
            outs = _as_list(outs)
            assert all(float(o.detach().abs().max()) == 0.0 for o in outs)
            sum(o.sum() for o in outs).backward()
            assert feat.grad.shape == feat.shape


def _warm_up(fn, times=3):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(times):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


def test_graph_capture_forward_and_backward():
    """gather forward + backward and raw splat forward + backward, each captured once and replayed on new values: the gather's result
    and every stored gradient equal the eager ones to the bit, what is summed with atomics to the bar"""
    dev, c = _dev(), PG.case("triplane_c16")
    grids = [g.to(dev).requires_grad_(True) for g in c["grids"]]
    pts = c["pts"].to(dev).requires_grad_(True)
    feat = c["vec"].to(dev).requires_grad_(True)
    vec, ups, gidx = c["vec"].to(dev), [u.to(dev) for u in c["up_grids"]], c["gidx"].to(dev)
    leaves = grids + [pts, feat]
    static = {}

    def step():
        for t in leaves:
            t.grad = None
        out = _gather(c, grids, None, pts, gidx)
        (out * vec).sum().backward()
        static["gather"], static["d_grids"], static["d_pts_gather"] = out.detach(), [g.grad for g in grids], pts.grad
        pts.grad = None
        outs = _splat(c, pts, feat, False, gidx)
        sum((o * u).sum() for o, u in zip(outs, ups)).backward()
        static["splat"], static["d_feat"], static["d_pts_splat"] = [o.detach() for o in outs], feat.grad, pts.grad

    _warm_up(step)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    captured = dict(static)  # (the tensors the captured graph writes)
    gen = torch.Generator().manual_seed(78)
    for round_ in range(2):
        if round_ == 1:  # new values in the tensors the graph reads
            with torch.no_grad():
                for g in grids:
                    g.copy_(0.5 * torch.randn(g.shape, generator=gen))
                feat.copy_(torch.randn(feat.shape, generator=gen))
        graph.replay()
        torch.cuda.synchronize()
        replayed = {k: [t.clone() for t in v] if isinstance(v, list) else v.clone() for k, v in captured.items()}
        step()
        for key in ("gather", "d_pts_gather", "d_feat", "d_pts_splat"):
            assert torch.equal(replayed[key], static[key]), f"round {round_}: replayed {key} != eager"
        for key in ("d_grids", "splat"):
            for i, (a, b) in enumerate(zip(replayed[key], static[key])):
                _worst(f"round {round_}: replayed {key}[{i}] vs eager", a, b)
    assert float((static["gather"].cpu().double() - c["gather"]).abs().max()) > 1e-3  # (the second round really saw other grids)

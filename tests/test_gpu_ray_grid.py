"""The fused weighted splat / gather along rays (lightplane_amd/ray_grid.py, csrc/lp_ray_grid.hip) against its fp64 definition.

Oracle, inputs, and the samples whose weight is zeroed: tests/ray_grid_cases.py (its docstring states every condition and cap;
tests/test_ray_grid_host.py::test_exclusion_caps_hold checks them without a GPU).  Every comparison is held to the project's bar,
max |err| / max |ref| <= 1e-4 per tensor, and prints its figure before it asserts.
"""
import itertools

import pytest
import torch

import lightplane_amd as lp
from tests import ray_grid_cases as RG
from tests.synth import random_rays
from tests.test_gpu_parity import _dev

pytestmark = pytest.mark.gpu

ALL = list(RG.CASES)
NORMALISED = [n for n in ALL if RG.CASES[n][6] == "pos"]
BAR_ATOMIC = 2e-5  # tests/test_gpu_partial_grads.py: the same sums in another order


def _worst(name, got, want, keep=None, tol=RG.TOL):
    """max |err| / max |ref| over the kept entries, printed and held to the bar"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    if keep is not None:
        k = keep.reshape(keep.shape + (1,) * (want.ndim - keep.ndim)).expand_as(want)
        got, want = got[k], want[k]
    scale = max(float(want.abs().max()), 1e-30)
    err = float((got - want).abs().max()) / scale
    print(f"{name}: max |err| / max |ref| = {err:.3e} (max |ref| {scale:.4g})")
    assert err <= tol, f"{name}: {err:.3e} > {tol}"


def _as_list(g):
    return g if isinstance(g, list) else [g]


def _rays(c, dev, origins=None, directions=None, gidx=None):
    n = len(c["gidx"])
    return lp.Rays(directions=c["directions"].to(dev) if directions is None else directions,
                   origins=c["origins"].to(dev) if origins is None else origins, grid_idx=c["gidx"].to(dev) if gidx is None else gidx,
                   near=torch.zeros(n, device=dev), far=torch.ones(n, device=dev))


def _gather(c, grid, sizes, depths, weights, rays=None):
    return lp.gather_along_rays(_rays(c, depths.device) if rays is None else rays, depths, weights, grid,
                                mask_out_of_bounds_samples=c["mask"], contract_coords=c["contract"], grid_sizes=sizes)


def _splat(c, depths, weights, feat, normalize, rays=None, as_list=None):
    as_list = c["form"] == "list" if as_list is None else as_list
    out = lp.splat_along_rays(_rays(c, depths.device) if rays is None else rays, depths, weights, feat, c["sizes"],
                              mask_out_of_bounds_samples=c["mask"], contract_coords=c["contract"], normalize=normalize, return_list=as_list)
    assert isinstance(out, list) == as_list
    return _as_list(out)


@pytest.mark.parametrize("name", ALL)
def test_gather_values(name):
    dev, c = _dev(), RG.case(name)
    grid, sizes = RG.grid_arg(c, c["grids"], dev)
    t, w = c["depths"].to(dev), c["w_kept"].to(dev)
    out = _gather(c, grid, sizes, t, w)
    assert out.shape == tuple(c["feat"].shape) and out.dtype == torch.float32 and out.device == dev
    _worst(f"{name} gather", out, c["gather"])
    assert torch.equal(_gather(c, grid, sizes, t, w), out), "a second call differs (the gather has no atomics)"
    other = dict(c, form="flat" if c["form"] == "list" else "list")
    grid2, sizes2 = RG.grid_arg(other, c["grids"], dev)
    assert torch.equal(_gather(c, grid2, sizes2, t, w), out), "the list and the flat form of the same grids differ"


@pytest.mark.parametrize("name", ALL)
def test_gather_gradients(name):
    dev, c = _dev(), RG.case(name)
    grid, sizes = RG.grid_arg(c, c["grids"], dev, requires_grad=True)
    g_out = c["g_out"].to(dev)
    w = c["w_kept"].to(dev).requires_grad_(True)
    out = _gather(c, grid, sizes, c["depths"].to(dev), w)
    grads = torch.autograd.grad(out, _as_list(grid) + [w], g_out)
    for i, (got, want) in enumerate(zip(grads[:-1], RG.in_form(c, c["gather_d_grid"]))):
        _worst(f"{name} gather: d grid[{i}]", got, want)
    _worst(f"{name} gather: d weights", grads[-1], c["gather_d_weights"], ~c["left_out"])
    t = c["depths"].to(dev).requires_grad_(True)
    out = _gather(c, [g.to(dev) for g in c["grids"]], None, t, c["w_live"].to(dev))
    (d_t,) = torch.autograd.grad(out, t, g_out)
    _worst(f"{name} gather: d depths", d_t, c["gather_d_depths"])


@pytest.mark.parametrize("name", ALL)
def test_splat_values(name):
    dev, c = _dev(), RG.case(name)
    t, w, f = c["depths"].to(dev), c["w_kept"].to(dev), c["feat"].to(dev)
    raw = _splat(c, t, w, f, False)
    for i, (got, want) in enumerate(zip(raw, RG.in_form(c, c["splat_raw"]))):
        _worst(f"{name} raw splat[{i}]", got, want)
    results = [raw]
    if c["normalize"]:
        norm = _splat(c, t, w, f, True)
        for i, (got, want) in enumerate(zip(norm, RG.in_form(c, c["splat_norm"]))):
            _worst(f"{name} normalised splat[{i}]", got, want)
        results.append(norm)
        untouched = [ws.reshape(-1) == 0 for ws in RG.in_form(c, c["w_sum"])]  # (positive weights: a touched row has a positive sum)
        n_untouched = sum(int(u.sum()) for u in untouched)
        for got in results:
            for g, u in zip(got, untouched):
                rows = g.reshape(u.numel(), -1).cpu()[u]
                assert rows.numel() == 0 or float(rows.abs().max()) == 0.0, "a row no sample touches is not exactly 0"
        print(f"{name}: {n_untouched} untouched rows are exactly 0")
    # the other return form holds the same numbers
    other = _splat(c, t, w, f, False, as_list=c["form"] != "list")
    flat = lambda gs: torch.cat([g.reshape(-1, g.shape[-1]) for g in gs])  # noqa: E731
    _worst(f"{name} raw splat, other return form", flat(other), flat(raw).cpu(), tol=BAR_ATOMIC)


@pytest.mark.parametrize("name", ALL)
def test_splat_gradients(name):
    dev, c = _dev(), RG.case(name)
    ups = [u.to(dev) for u in RG.in_form(c, c["up_grids"])]
    t = c["depths"].to(dev)
    for normalize, want in ((False, c["splat_d_feat"]), (True, c["splat_d_feat_norm"])):
        if normalize and not c["normalize"]:
            continue
        f = c["feat"].to(dev).requires_grad_(True)
        outs = _splat(c, t, c["w_kept"].to(dev), f, normalize)
        sum((o * u).sum() for o, u in zip(outs, ups)).backward()
        _worst(f"{name} splat (normalize={normalize}): d features", f.grad, want)
    w = c["w_kept"].to(dev).requires_grad_(True)
    outs = _splat(c, t, w, c["feat"].to(dev), False)
    sum((o * u).sum() for o, u in zip(outs, ups)).backward()
    _worst(f"{name} raw splat: d weights", w.grad, c["splat_d_weights"], ~c["left_out"])
    t = c["depths"].to(dev).requires_grad_(True)
    outs = _splat(c, t, c["w_live"].to(dev), c["feat"].to(dev), False)
    sum((o * u).sum() for o, u in zip(outs, ups)).backward()
    _worst(f"{name} raw splat: d depths", t.grad, c["splat_d_depths"])


@pytest.mark.parametrize("name", ALL)
def test_gather_and_splat_are_adjoint(name):
    """from GPU results alone, both sides summed in fp64: <gather(G, W), F> = <G, splat(W, F)>"""
    dev, c = _dev(), RG.case(name)
    grids = [g.to(dev) for g in c["grids"]]
    t, w, f = c["depths"].to(dev), c["w_kept"].to(dev), c["feat"].to(dev)
    gathered = _gather(c, grids, None, t, w)
    splatted = _splat(c, t, w, f, False, as_list=True)
    lhs = gathered.double() * f.double()
    rhs = [g.double() * s.double() for g, s in zip(grids, splatted)]
    a, b = float(lhs.sum()), float(sum(r.sum() for r in rhs))
    scale = min(float(lhs.abs().sum()), float(sum(r.abs().sum() for r in rhs)))
    print(f"{name}: <gather, F> = {a:.9g}, <G, splat> = {b:.9g}, |difference| / sum |products| = {abs(a - b) / scale:.3e}")
    assert abs(a - b) <= RG.TOL * scale


@pytest.mark.parametrize("name", ["triplane_c16", "voxel_c5_mask", "triplane_c20_contract_mask", "dense_ray", "signed_weights"])
def test_agrees_with_the_point_ops(name):
    """the composition through the [R, S, C] tensors: splat_points / sample_grid_at_points at o + t d"""
    dev, c = _dev(), RG.case(name)
    grids = [g.to(dev) for g in c["grids"]]
    o, d, t, w, f, gidx = (c[k].to(dev) for k in ("origins", "directions", "depths", "w_kept", "feat", "gidx"))
    pts = t[..., None] * d[:, None, :] + o[:, None, :]
    want = lp.splat_points(pts, (w[..., None] * f[:, None]).contiguous(), c["sizes"], gidx, c["mask"], c["contract"], normalize=False)
    got = _splat(c, t, w, f, False, as_list=True)
    for i, (a, b) in enumerate(zip(got, want)):
        _worst(f"{name} splat_along_rays vs splat_points, grid {i}", a, b)
    want = (lp.sample_grid_at_points(pts, grids, gidx, c["mask"], c["contract"]) * w[..., None]).sum(1)
    _worst(f"{name} gather_along_rays vs sample_grid_at_points", _gather(c, grids, None, t, w), want)


def test_unit_weights_at_the_splatters_depths_are_the_splatter():
    """weights = 1 at the depths of ray_samples, normalised: lightplane_splatter on the same rays (64 rays, 16 samples)"""
    dev = _dev()
    gen = torch.Generator().manual_seed(41)
    sizes = [[2, 6, 5, 7, 16], [2, 1, 6, 7, 16]]
    rays = random_rays(gen, 64, 2, 16).to(dev)
    depths = lp.ray_samples(rays, 16).depths
    want = lp.lightplane_splatter(rays, sizes, num_samples=16)
    got = lp.splat_along_rays(rays, depths, torch.ones_like(depths), rays.encoding, sizes, normalize=True)
    for i, (g, w) in enumerate(zip(got, want)):
        assert float(w.abs().max()) > 0
        _worst(f"splat_along_rays vs lightplane_splatter, grid {i}", g, w)


def test_masked_and_zero_weight_samples_add_exactly_nothing():
    dev = _dev()
    # the mask: the samples outside the box alone leave zero grids; with zero weights nothing changes to the bit for the stored results
    c = RG.case("voxel_c5_mask")
    inside = c["inside"].to(dev)
    assert 0 < int((~inside).sum()) < inside.numel() and int(c["left_out"].sum()) == 0
    t, w, f = c["depths"].to(dev), c["weights"].to(dev), c["feat"].to(dev)
    grids = [g.to(dev) for g in c["grids"]]
    w_out, w_in = w * (~inside).float(), w * inside.float()
    for normalize in (False, True):
        assert all(float(g.abs().max()) == 0.0 for g in _splat(c, t, w_out, f, normalize)), "samples outside the box added something"
    assert float(_gather(c, grids, None, t, w_out).abs().max()) == 0.0
    assert torch.equal(_gather(c, grids, None, t, w), _gather(c, grids, None, t, w_in))
    for a, b in zip(_splat(c, t, w, f, False), _splat(c, t, w_in, f, False)):
        _worst("voxel_c5_mask raw splat: all samples vs the samples inside", a, b, tol=BAR_ATOMIC)
    # ... and they get nothing: the sample gradients outside are exactly 0
    tt, ww = t.clone().requires_grad_(True), w.clone().requires_grad_(True)
    (_gather(c, grids, None, tt, ww) * c["g_out"].to(dev)).sum().backward()
    for g in (tt.grad, ww.grad):
        assert float(g[~inside].abs().max()) == 0.0 and float(g[inside].abs().max()) > 0.0
    # zero weights without a mask: a ray of zeros leaves zero grids; zero-weight samples leave the gather as it is
    c = RG.case("signed_weights")
    t, w, f = c["depths"].to(dev), c["weights"].to(dev), c["feat"].to(dev)
    assert all(float(g.abs().max()) == 0.0 for g in _splat(c, t, torch.zeros_like(w), f, False))
    grids = [g.to(dev) for g in c["grids"]]
    far = torch.where(w == 0, torch.full_like(t, 0.37), t)  # (a zero-weight sample may sit anywhere)
    assert torch.equal(_gather(c, grids, None, far, w), _gather(c, grids, None, t, w))


def _subsets(names):
    return [s for k in range(1, len(names) + 1) for s in itertools.combinations(names, k)]


def test_gather_partial_gradients():
    dev, c = _dev(), RG.case("triplane_c16")
    g_out = c["g_out"].to(dev)

    def run(subset):
        grids = [g.to(dev).requires_grad_("grids" in subset) for g in c["grids"]]
        t = c["depths"].to(dev).requires_grad_("depths" in subset)
        w = c["weights"].to(dev).requires_grad_("weights" in subset)
        out = _gather(c, grids, None, t, w)
        (out * g_out).sum().backward()
        return out.detach(), grids, t, w

    names = ("grids", "depths", "weights")
    ref_out, ref_grids, ref_t, ref_w = run(names)
    for subset in _subsets(names):
        out, grids, t, w = run(subset)
        assert torch.equal(out, ref_out), subset
        for key, got, ref in (("depths", t, ref_t), ("weights", w, ref_w)):
            if key in subset:
                assert torch.equal(got.grad, ref.grad), f"{subset}: the stored gradient of {key} differs"
            else:
                assert got.grad is None, f"{subset}: {key} did not ask and got a gradient"
        for i, (g, r) in enumerate(zip(grids, ref_grids)):
            if "grids" in subset:
                _worst(f"{subset}: d grid[{i}] vs all leaves", g.grad, r.grad, tol=BAR_ATOMIC)
            else:
                assert g.grad is None, f"{subset}: grid {i} did not ask and got a gradient"
    # one grid of the list alone
    grids = [g.to(dev).requires_grad_(i == 1) for i, g in enumerate(c["grids"])]
    (_gather(c, grids, None, c["depths"].to(dev), c["weights"].to(dev)) * g_out).sum().backward()
    assert grids[0].grad is None and grids[2].grad is None
    _worst("only grid 1 asks: d grid[1] vs all leaves", grids[1].grad, ref_grids[1].grad, tol=BAR_ATOMIC)


def test_splat_partial_gradients():
    dev, c = _dev(), RG.case("triplane_c16")
    ups = [u.to(dev) for u in c["up_grids"]]

    def run(subset, normalize=False):
        f = c["feat"].to(dev).requires_grad_("features" in subset)
        t = c["depths"].to(dev).requires_grad_("depths" in subset)
        w = c["weights"].to(dev).requires_grad_("weights" in subset)
        outs = _splat(c, t, w, f, normalize)
        sum((o * u).sum() for o, u in zip(outs, ups)).backward()
        return [o.detach() for o in outs], dict(features=f, depths=t, weights=w)

    names = ("features", "depths", "weights")
    ref_outs, ref = run(names)
    for subset in _subsets(names):
        outs, leaves = run(subset)
        for i, (o, r) in enumerate(zip(outs, ref_outs)):  # (summed with atomics: the order differs from call to call)
            _worst(f"{subset}: splat[{i}] vs all leaves", o, r, tol=BAR_ATOMIC)
        for key in names:
            if key in subset:
                assert torch.equal(leaves[key].grad, ref[key].grad), f"{subset}: the stored gradient of {key} differs"
            else:
                assert leaves[key].grad is None, f"{subset}: {key} did not ask and got a gradient"
    _, leaves = run(("features",), normalize=True)
    _worst("normalised splat, features alone: d features", leaves["features"].grad, c["splat_d_feat_norm"])
    assert torch.equal(c["w_kept"], c["weights"])  # (no mask: the oracle's weights are the case's)
    # only one of the returned grids is differentiated: the others count as zero upstream gradients
    f = c["feat"].to(dev).requires_grad_(True)
    outs = _splat(c, c["depths"].to(dev), c["weights"].to(dev), f, False)
    (outs[1] * ups[1]).sum().backward()
    only = [torch.zeros_like(u) if i != 1 else u for i, u in enumerate(ups)]
    want = _gather(c, only, None, c["depths"].to(dev), c["weights"].to(dev))
    assert torch.equal(f.grad, want), "only splat[1] is differentiated: d features is not the gather of that upstream alone"


def _offset(t):
    """the values of ``t`` as a dense view one element into a larger buffer (4-byte aligned only)"""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _strided(t):
    """the values of ``t`` as a non-contiguous view: every other row of a tensor twice as long, the leading columns of a wider one"""
    if t.ndim == 1:
        v = torch.zeros(2 * t.shape[0], dtype=t.dtype, device=t.device)[::2]
    else:
        v = torch.zeros(2 * t.shape[0], t.shape[1] + 3, dtype=t.dtype, device=t.device)[::2, :t.shape[1]]
    v.copy_(t)
    assert not v.is_contiguous()
    return v


def test_views_give_the_contiguous_result():
    dev, c = _dev(), RG.case("triplane_c16")
    base = dict(origins=c["origins"].to(dev), directions=c["directions"].to(dev), gidx=c["gidx"].to(dev), depths=c["depths"].to(dev),
                weights=c["weights"].to(dev), feat=c["feat"].to(dev))
    grids = [g.to(dev) for g in c["grids"]]
    g_out, ups = c["g_out"].to(dev), [u.to(dev) for u in c["up_grids"]]

    def run(v, gs, upstream=g_out, up_grids=ups):
        rays = _rays(c, dev, v["origins"], v["directions"], v["gidx"])
        t, w, f = (v[k].detach().requires_grad_(True) for k in ("depths", "weights", "feat"))
        gs = [g.detach().requires_grad_(True) for g in gs]
        out = _gather(c, gs, None, t, w, rays)
        (out * upstream).sum().backward()
        stored = [out.detach(), t.grad, w.grad]
        summed = [g.grad for g in gs]
        t.grad = w.grad = None
        outs = _splat(c, t, w, f, False, rays)
        sum((o * u).sum() for o, u in zip(outs, up_grids)).backward()
        return stored + [f.grad, t.grad, w.grad], summed + [o.detach() for o in outs]

    ref_stored, ref_summed = run(base, grids)
    variants = [(f"{k} {kind.__name__}", dict(base, **{k: kind(base[k])}), grids, g_out, ups) for k in base for kind in (_offset, _strided)]
    variants += [(f"grid[{i}] _offset", base, [(_offset(g) if j == i else g) for j, g in enumerate(grids)], g_out, ups) for i in range(len(grids))]
    variants += [("upstream of the gather _strided", base, grids, _strided(g_out), ups), ("upstream of the gather _offset", base, grids, _offset(g_out), ups),
                 ("upstream of the splat _offset", base, grids, g_out, [_offset(u) for u in ups])]
    for tag, v, gs, upstream, up_grids in variants:
        stored, summed = run(v, gs, upstream, up_grids)
        for i, (a, b) in enumerate(zip(stored, ref_stored)):
            assert torch.equal(a, b), f"{tag}: stored result {i} differs from the contiguous call"
        for i, (a, b) in enumerate(zip(summed, ref_summed)):
            _worst(f"{tag}: summed result {i} vs the contiguous call", a, b, tol=BAR_ATOMIC)


@pytest.mark.parametrize("shape", [(0, 5), (4, 0)])
def test_empty_batches(shape):
    dev, c = _dev(), RG.case("triplane_c16")
    R, S = shape
    grids = [g.to(dev).requires_grad_(True) for g in c["grids"]]
    rays = lp.Rays(directions=torch.ones(R, 3, device=dev), origins=torch.zeros(R, 3, device=dev),
                   grid_idx=torch.zeros(R, dtype=torch.long, device=dev), near=torch.zeros(R, device=dev), far=torch.ones(R, device=dev))
    t = torch.zeros(R, S, device=dev, requires_grad=True)
    w = torch.ones(R, S, device=dev, requires_grad=True)
    out = lp.gather_along_rays(rays, t, w, grids)
    assert out.shape == (R, 16) and (out.numel() == 0 or float(out.detach().abs().max()) == 0.0)
    out.sum().backward()
    assert t.grad.shape == (R, S) and w.grad.shape == (R, S) and all(float(g.grad.abs().max()) == 0.0 for g in grids)
    for normalize in (False, True):
        for as_list in (True, False):
            f = torch.ones(R, 16, device=dev, requires_grad=True)
            tt, ww = (t.detach(), w.detach()) if normalize else (t.detach().requires_grad_(True), w.detach().requires_grad_(True))
            outs = lp.splat_along_rays(rays, tt, ww, f, c["sizes"], normalize=normalize, return_list=as_list)
            if as_list:
                assert [list(o.shape) for o in outs] == c["sizes"]
            else:
                assert outs.shape == (sum(s[0] * s[1] * s[2] * s[3] for s in c["sizes"]), 16)
            outs = _as_list(outs)
            assert all(float(o.detach().abs().max()) == 0.0 for o in outs)
            sum(o.sum() for o in outs).backward()
            assert f.grad.shape == f.shape and (f.grad.numel() == 0 or float(f.grad.abs().max()) == 0.0)
            if not normalize:
                assert tt.grad.shape == (R, S) and ww.grad.shape == (R, S)


def _warm_up(fn, times=3):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(times):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


def test_graph_capture_forward_and_backward():
    """gather forward + backward and raw splat forward + backward, captured once and replayed on new values: the gather's result and every
    stored gradient equal the eager ones to the bit, what is summed with atomics to the bar of such sums"""
    dev, c = _dev(), RG.case("voxel_c32_flat")
    c = dict(c, form="list")
    grids = [g.to(dev).requires_grad_(True) for g in c["grids"]]
    t = c["depths"].to(dev).requires_grad_(True)
    w = c["weights"].to(dev).requires_grad_(True)
    f = c["feat"].to(dev).requires_grad_(True)
    g_out, ups, rays = c["g_out"].to(dev), [u.to(dev) for u in c["up_grids"]], _rays(c, dev)
    leaves = grids + [t, w, f]
    static = {}

    def step():
        for x in leaves:
            x.grad = None
        out = _gather(c, grids, None, t, w, rays)
        (out * g_out).sum().backward()
        static["gather"], static["d_grids"], static["d_t_gather"], static["d_w_gather"] = out.detach(), [g.grad for g in grids], t.grad, w.grad
        t.grad = w.grad = None
        outs = _splat(c, t, w, f, False, rays)
        sum((o * u).sum() for o, u in zip(outs, ups)).backward()
        static["splat"], static["d_feat"], static["d_t_splat"], static["d_w_splat"] = [o.detach() for o in outs], f.grad, t.grad, w.grad

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
                f.copy_(torch.randn(f.shape, generator=gen))
                w.copy_(0.1 + torch.rand(w.shape, generator=gen))
        graph.replay()
        torch.cuda.synchronize()
        replayed = {k: [x.clone() for x in v] if isinstance(v, list) else v.clone() for k, v in captured.items()}
        step()
        for key in ("gather", "d_t_gather", "d_w_gather", "d_feat", "d_t_splat", "d_w_splat"):
            assert torch.equal(replayed[key], static[key]), f"round {round_}: replayed {key} != eager"
        for key in ("d_grids", "splat"):
            for i, (a, b) in enumerate(zip(replayed[key], static[key])):
                _worst(f"round {round_}: replayed {key}[{i}] vs eager", a, b, tol=BAR_ATOMIC)
    assert float((static["gather"].cpu().double() - c["gather"]).abs().max()) > 1e-3  # (the second round really saw other values)

"""The fused space-time plane encoding (lightplane_amd/kplanes.py, csrc/lp_kplanes.hip) against its definition: ``reference`` below, the
module docstring's lines in torch fp64 on the fp32 inputs with plain indexing, differentiated with autograd; every tensor to
max |err| / max |ref| <= 1e-4.  Exclusions are conditions on the fp64 inputs, as in tests/test_gpu_hash_grid.py, with its thresholds and
caps (tests/test_kplanes_host.py holds the caps); nothing is excluded from unmasked values or from the plane gradient.  Measured worst
errors: DESIGN.md 4.25."""
import pytest
import torch

import lightplane_amd as lp
from tests.test_gpu_hash_grid import FACE_EPS, INT_EPS, KINK_EPS, MAX_LEFT_OUT, MAX_ZEROED, _contract  # noqa: F401 (the caps: for the host test)
from tests.test_gpu_parity import _dev
from tests.test_gpu_ray_grid import BAR_ATOMIC, _warm_up, _worst   # the bar (1e-4), printed before it is held; 2e-5 for reordered sums

pytestmark = pytest.mark.gpu

AXES = ((0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (2, 3))   # xy, xz, yz, xt, yt, zt over (x, y, z, t)
DYN = dict(resolutions=(5, 9), time_resolution=(4, 4), channels=8)
#   name: layout, (R, N), batch, how the points are drawn (half-width of a cube | "cell" | "ray"), mask, contract, times per point
CASES = {
    "dynamic": (DYN, (7, 37), 2, 1.2, False, False, False),
    "static": (dict(DYN, time_resolution=None), (7, 37), 2, 1.2, False, False, False),
    "c4": (dict(DYN, channels=4), (7, 37), 2, 1.2, False, False, False),
    "c64": (dict(DYN, channels=64), (7, 37), 2, 1.2, False, False, False),
    "kplanes_128": (dict(resolutions=(4, 8, 16, 32), time_resolution=6, channels=32), (7, 37), 2, 1.2, False, False, False),
    "point_times": (DYN, (7, 37), 2, 1.2, False, False, True),
    "min_res": (dict(DYN, resolutions=(2,), time_resolution=(2,)), (7, 37), 2, 1.2, False, False, False),
    "zeros": (DYN, (7, 37), 2, 1.2, False, False, False),
    "masked": (DYN, (7, 37), 2, 1.2, True, False, False),   # (a contracted point never leaves the cube: the mask alone removes some)
    "masked_contracted": (DYN, (7, 37), 2, 3.0, True, True, False),
    "one_cell": (DYN, (1, 64), 1, "cell", False, False, False),
    "along_ray": (DYN, (1, 200), 1, "ray", False, False, False),
    "one_point": (DYN, (1, 1), 2, 1.2, False, False, False),
}
SEEDS = {name: 1300 + i for i, name in enumerate(CASES)}
ALL = list(CASES)
_CACHE = {}


def _coords(q, times):
    """the (x, y, z[, t]) coordinates of every point, each [R, N]"""
    c = list(q.unbind(-1))
    if times is not None:
        c.append(times if times.ndim == 2 else times[:, None].expand(q.shape[:2]))
    return c


def reference(points, times, planes, gidx, lay, mask, contract, touched=None):
    """the definition, in the dtype of ``points`` / ``planes`` (fp64 here); ``touched [B, rows]`` (bool) is set where a point reads"""
    q = _contract(points) if contract else points
    inside = (q.abs() <= 1.0).all(-1) if mask else torch.ones(q.shape[:2], dtype=torch.bool)
    b = gidx.long().clamp(0, planes.shape[0] - 1)[:, None].expand(points.shape[:2])
    coords, out = _coords(q, times), []
    for s in range(lay.n_scales):
        res = [lay.spatial[s]] * 3 + ([lay.temporal[s]] if lay.temporal else [])
        x = [(c * ((n - 1) / 2) + (n - 1) / 2).clamp(0, n - 1) for c, n in zip(coords, res)]
        i = [xa.detach().floor().clamp(max=n - 2).long() for xa, n in zip(x, res)]
        f = [xa - ia for xa, ia in zip(x, i)]
        prod = 1
        for j, (u, v) in enumerate(AXES[:lay.n_planes]):
            val = 0
            for ku, kv in ((0, 0), (1, 0), (0, 1), (1, 1)):
                w = (f[u] if ku else 1 - f[u]) * (f[v] if kv else 1 - f[v])
                row = lay.offsets[s][j] + i[u] + ku + res[u] * (i[v] + kv)
                val = val + w[..., None] * planes[b, row]
                if touched is not None:
                    touched[b[inside], row[inside]] = True
            prod = prod * val
        out.append(prod)
    return torch.cat(out, dim=-1) * inside[..., None]


def case(name):
    """inputs, exclusion masks and the fp64 results of a case: built once per process and never modified"""
    if name in _CACHE:
        return _CACHE[name]
    kw, (R, N), B, draw, mask, contract, per_point = CASES[name]
    lay = lp.kplanes_layout(**kw)
    gen = torch.Generator().manual_seed(SEEDS[name])
    if draw == "cell":    # inside cell (3, 6, 1) of the finest scale, at 0.1 .. 0.9 of the cell
        x = torch.tensor([3.0, 6.0, 1.0]) + 0.1 + 0.8 * torch.rand(R, N, 3, generator=gen)
        pts = 2 * x / (lay.spatial[-1] - 1) - 1
    elif draw == "ray":   # sorted depths along one ray through the box
        t = torch.rand(R, N, generator=gen).sort(dim=1).values
        pts = torch.tensor([-0.9, -0.7, -0.8]) + t[..., None] * torch.tensor([1.7, 1.5, 1.2])
    else:
        pts = (torch.rand(R, N, 3, generator=gen) * 2 - 1) * draw
    times = None
    if lay.n_planes == 6:
        times = (torch.rand((R, N) if per_point else (R,), generator=gen) * 2 - 1) * (0.8 if draw in ("cell", "ray") else 1.2)
    gidx = torch.tensor([0, 1, 1, 0, 5, -2, 1][:R]) if B > 1 else torch.zeros(R, dtype=torch.int64)
    shape = (B, lay.rows, lay.channels)   # magnitudes in [0.5, 1.5], one sign per (scene, channel): a product of six stays in range
    planes = (0.5 + torch.rand(shape, generator=gen)) * (torch.randint(0, 2, (B, 1, lay.channels), generator=gen) * 2 - 1)
    if name == "zeros":   # a third of the entries exactly 0, and every row of the xy plane of scale 0
        planes[torch.rand(shape, generator=gen) < 1 / 3] = 0.0
        planes[:, lay.offsets[0][0]:lay.offsets[0][1]] = 0.0
    up = torch.randn(R, N, lay.out_channels, generator=gen)

    p64, t64 = pts.double(), None if times is None else times.double()
    a = p64.abs().sort(dim=-1, descending=True).values
    q64 = _contract(p64) if contract else p64
    zeroed = torch.zeros(R, N, dtype=torch.bool)
    if contract:
        zeroed |= ((a[..., 0] - 1.0).abs() < KINK_EPS) | ((a[..., 0] > 1.0) & ((a[..., 0] - a[..., 1]) < KINK_EPS))
    for s in range(lay.n_scales):
        for c, n in zip(_coords(q64, t64), [lay.spatial[s]] * 3 + ([lay.temporal[s]] if lay.temporal else [])):
            x = ((c + 1) / 2 * (n - 1)).clamp(-0.5, n - 0.5)   # (a coordinate clamped away has no kink)
            zeroed |= (x - x.round()).abs() < INT_EPS
    left_out = ((q64.abs() - 1.0).abs() < FACE_EPS).any(-1) if mask else torch.zeros(R, N, dtype=torch.bool)
    zeroed |= left_out
    up_live = up * (~zeroed)[..., None]

    p, pl64, touched = p64.clone().requires_grad_(True), planes.double().requires_grad_(True), torch.zeros(B, lay.rows, dtype=torch.bool)
    want = reference(p, t64, pl64, gidx, lay, mask, contract, touched)
    (d_planes,) = torch.autograd.grad(want, pl64, up.double(), retain_graph=True)
    (d_points,) = torch.autograd.grad(want, p, up_live.double())
    inside = (q64.abs() <= 1.0).all(-1) | (not mask)
    _CACHE[name] = dict(lay=lay, pts=pts, times=times, gidx=gidx, planes=planes, up=up, up_live=up_live, mask=mask, contract=contract,
                        zeroed=zeroed, left_out=left_out, inside=inside, want=want.detach(), d_planes=d_planes, d_points=d_points,
                        untouched=~touched)
    return _CACHE[name]


def _encode(c, pts, planes, gidx=None, times=None):
    times = times if times is not None else (None if c["times"] is None else c["times"].to(pts.device))
    return lp.kplanes_encode(pts, times, planes, c["gidx"].to(pts.device) if gidx is None else gidx, c["lay"],
                             mask_out_of_bounds_samples=c["mask"], contract_coords=c["contract"])


@pytest.mark.parametrize("name", ALL)
def test_values(name):
    dev, c = _dev(), case(name)
    pts, planes = c["pts"].to(dev), c["planes"].to(dev)
    out = _encode(c, pts, planes)
    assert out.shape == c["want"].shape and out.dtype == torch.float32 and out.device == dev
    _worst(f"{name} values", out, c["want"], ~c["left_out"])
    assert torch.equal(_encode(c, pts, planes), out), "a second call differs (the forward has no atomics)"
    assert float(out.cpu()[~c["inside"] & ~c["left_out"]].abs().sum()) == 0.0, "a masked point has a feature that is not exactly 0"


@pytest.mark.parametrize("name", ALL)
def test_gradients(name):
    dev, c = _dev(), case(name)
    pts, planes = c["pts"].to(dev).requires_grad_(True), c["planes"].to(dev).requires_grad_(True)
    out = _encode(c, pts, planes)
    (d_planes,) = torch.autograd.grad(out, planes, c["up"].to(dev), retain_graph=True)
    assert bool(torch.isfinite(d_planes).all())
    _worst(f"{name} d planes", d_planes, c["d_planes"])
    assert float(d_planes.cpu()[c["untouched"]].abs().sum()) == 0.0, "a row no point touches is not exactly 0"
    (d_pts,) = torch.autograd.grad(out, pts, c["up_live"].to(dev), retain_graph=True)
    assert bool(torch.isfinite(d_pts).all())
    _worst(f"{name} d points", d_pts, c["d_points"])
    assert torch.equal(torch.autograd.grad(out, pts, c["up_live"].to(dev), retain_graph=True)[0], d_pts), "a second point gradient differs"
    gone = ~c["inside"] & ~c["left_out"]
    assert float(d_pts.cpu()[gone].abs().sum()) == 0.0, "a masked point has a gradient"
    (g,) = torch.autograd.grad(out, planes, c["up"].to(dev) * gone.to(dev)[..., None])   # the masked points alone
    assert float(g.abs().sum()) == 0.0, "masked points add to the plane gradient"


@pytest.mark.parametrize("name", ["dynamic", "c64", "masked_contracted"])
@pytest.mark.parametrize("which", ["planes", "points"])
def test_only_some_gradients(name, which):
    dev, c = _dev(), case(name)
    pts, planes = c["pts"].to(dev).requires_grad_(which == "points"), c["planes"].to(dev).requires_grad_(which == "planes")
    out = _encode(c, pts, planes)
    assert torch.equal(out, _encode(c, pts.detach(), planes.detach())), "the forward depends on who asks for a gradient"
    (out * c["up_live"].to(dev)).sum().backward()
    asked, other = (planes, pts) if which == "planes" else (pts, planes)
    assert other.grad is None
    full_p, full_t = c["pts"].to(dev).requires_grad_(True), c["planes"].to(dev).requires_grad_(True)
    (_encode(c, full_p, full_t) * c["up_live"].to(dev)).sum().backward()
    if which == "points":
        assert torch.equal(asked.grad, full_p.grad)
    else:
        _worst(f"{name}: d planes alone vs with the point gradient", asked.grad, full_t.grad, tol=BAR_ATOMIC)


@pytest.mark.parametrize("shape", [(0, 5), (3, 0)])
def test_empty_batch(shape):
    dev, c = _dev(), case("dynamic")
    pts = torch.zeros(shape + (3,), device=dev, requires_grad=True)
    planes = c["planes"].to(dev).requires_grad_(True)
    out = _encode(c, pts, planes, torch.zeros(shape[0], dtype=torch.int64, device=dev), torch.zeros(shape[0], device=dev))
    assert out.shape == shape + (c["lay"].out_channels,)
    out.sum().backward()
    assert planes.grad.shape == planes.shape and float(planes.grad.abs().sum()) == 0.0 and pts.grad.shape == pts.shape


def test_times_gradient_is_refused():
    dev, c = _dev(), case("dynamic")
    with pytest.raises(NotImplementedError, match=r"\.detach\(\)"):
        _encode(c, c["pts"].to(dev), c["planes"].to(dev), times=c["times"].to(dev).requires_grad_())


def test_graph_capture_forward_and_backward():
    """captured once, replayed on new values: values and the point gradient to the bit, the plane gradient (atomics) to BAR_ATOMIC"""
    dev, c = _dev(), case("dynamic")
    pts, planes = c["pts"].to(dev).requires_grad_(True), c["planes"].to(dev).requires_grad_(True)
    up, gidx, times, static = c["up_live"].to(dev), c["gidx"].to(dev), c["times"].to(dev), {}

    def step():
        pts.grad = planes.grad = None
        out = _encode(c, pts, planes, gidx, times)
        (out * up).sum().backward()
        static["out"], static["d_pts"], static["d_planes"] = out.detach(), pts.grad, planes.grad

    _warm_up(step)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    captured = dict(static)
    gen = torch.Generator().manual_seed(79)
    for round_ in range(3):
        if round_:  # new values in the tensors the graph reads
            with torch.no_grad():
                planes.copy_(torch.randn(planes.shape, generator=gen))
                pts.copy_((torch.rand(pts.shape, generator=gen) * 2 - 1) * 1.2)
                times.copy_(torch.rand(times.shape, generator=gen) * 2 - 1)
        graph.replay()
        torch.cuda.synchronize()
        replayed = {k: v.clone() for k, v in captured.items()}
        step()
        for key in ("out", "d_pts"):
            assert torch.equal(replayed[key], static[key]), f"round {round_}: replayed {key} != eager"
        _worst(f"round {round_}: replayed d planes vs eager", replayed["d_planes"], static["d_planes"], tol=BAR_ATOMIC)
    assert float((static["out"].cpu().double() - c["want"]).abs().max()) > 1e-3  # (the later rounds really saw other values)

"""The fused hash-grid encoding (lightplane_amd/hash_grid.py, csrc/lp_hash_grid.hip) against its definition: ``reference`` below, the
module docstring's lines in torch fp64 on the fp32 inputs, differentiated with autograd; every tensor to max |err| / max |ref| <= 1e-4.
Exclusions are conditions on the fp64 inputs (tests/test_hash_grid_host.py holds their caps): for the POINT gradient only, a zero
upstream gradient where x = (q + 1) / 2 N_l is within 1e-4 of an integer on any level and axis, or on the contraction's kink
(tests/point_grid_cases.py's rule), <= 5 % of a case; with the mask, a point within 1e-5 of a cube face is left out of the value
comparisons, <= 2 %.  Nothing is excluded from unmasked values or from the table gradient.  A seed that misses a cap is changed."""
import pytest
import torch

import lightplane_amd as lp
from tests.test_gpu_parity import _dev
from tests.test_gpu_ray_grid import BAR_ATOMIC, _warm_up, _worst   # the bar (1e-4), printed before it is held; 2e-5 for reordered sums

pytestmark = pytest.mark.gpu

INT_EPS, KINK_EPS, FACE_EPS, MAX_ZEROED, MAX_LEFT_OUT = 1e-4, 1e-3, 1e-5, 0.05, 0.02
MIXED = dict(n_levels=4, features_per_level=2, log2_table_size=8, base_resolution=4, finest_resolution=32)
#   name: layout, (R, N), batch, how the points are drawn (half-width of a cube | "cell" | "ray"), mask, contract
CASES = {
    "mixed": (MIXED, (7, 37), 2, 1.2, False, False),
    "f1": (dict(MIXED, features_per_level=1), (7, 37), 2, 1.2, False, False),
    "f4": (dict(MIXED, features_per_level=4), (7, 37), 2, 1.2, False, False),
    "f8": (dict(MIXED, features_per_level=8), (7, 37), 2, 1.2, False, False),
    "one_level": (dict(MIXED, n_levels=1, base_resolution=1, finest_resolution=1), (7, 37), 2, 1.2, False, False),
    "collide": (dict(MIXED, n_levels=1, log2_table_size=3, base_resolution=64, finest_resolution=64), (7, 37), 2, 1.2, False, False),
    "ngp": (dict(n_levels=16, features_per_level=2, log2_table_size=10, base_resolution=16, finest_resolution=256), (7, 37), 2, 1.2, False, False),
    "masked": (MIXED, (7, 37), 2, 1.2, True, False),
    "masked_contracted": (MIXED, (7, 37), 2, 3.0, True, True),
    "one_cell": (MIXED, (1, 64), 1, "cell", False, False),
    "along_ray": (dict(MIXED, n_levels=3, base_resolution=2, finest_resolution=8), (1, 200), 1, "ray", False, False),
    "one_point": (MIXED, (1, 1), 2, 1.2, False, False),
}
SEEDS = {name: 900 + i for i, name in enumerate(CASES)}
ALL = list(CASES)
_CACHE = {}


def _contract(p):   # the Renderer's contraction, into [-1, 1]^3
    a = p.abs()
    n = a.max(dim=-1, keepdim=True).values
    return torch.where(n <= 1.0, p, torch.where((a - n).abs() <= 1e-7, (2 - 1 / a) * (p / a), p / n)) / 2


def reference(points, table, gidx, lay, mask, contract):
    """the definition, in the dtype of ``points`` / ``table`` (fp64 here), integer hashing in int64"""
    q = _contract(points) if contract else points
    b = gidx.long().clamp(0, table.shape[0] - 1)[:, None].expand(points.shape[:2])
    u = ((q + 1) / 2).clamp(0, 1)
    T, M32, out = 1 << lay.log2_table_size, (1 << 32) - 1, []
    for n_l, off, hashed in zip(lay.resolutions, lay.offsets, lay.hashed):
        x = u * n_l
        i = x.detach().floor().clamp(max=n_l - 1).long()
        f = x - i
        acc = 0
        for k in range(8):
            bits = torch.tensor([k & 1, (k >> 1) & 1, (k >> 2) & 1])
            cx, cy, cz = (i + bits).unbind(-1)
            w = torch.where(bits.bool(), f, 1 - f).prod(-1)
            if hashed:
                idx = (cx ^ ((cy * 2654435761) & M32) ^ ((cz * 805459861) & M32)) & (T - 1)
            else:
                idx = cx + (n_l + 1) * (cy + (n_l + 1) * cz)
            acc = acc + w[..., None] * table[b, off + idx]
        out.append(acc)
    out = torch.cat(out, dim=-1)
    return out * (q.abs() <= 1.0).all(-1, keepdim=True) if mask else out


def case(name):
    """inputs, exclusion masks and the fp64 results of a case: built once per process and never modified"""
    if name in _CACHE:
        return _CACHE[name]
    kw, (R, N), B, draw, mask, contract = CASES[name]
    lay = lp.hash_grid_layout(**kw)
    gen = torch.Generator().manual_seed(SEEDS[name])
    if draw == "cell":    # inside cell (10, 20, 5) of the finest level, away from its faces
        x = torch.tensor([10.0, 20.0, 5.0]) + 0.1 + 0.8 * torch.rand(R, N, 3, generator=gen)
        pts = 2 * x / lay.resolutions[-1] - 1
    elif draw == "ray":   # sorted depths along one ray through the box
        t = torch.rand(R, N, generator=gen).sort(dim=1).values
        pts = torch.tensor([-0.9, -0.7, -0.8]) + t[..., None] * torch.tensor([1.7, 1.5, 1.2])
    else:
        pts = (torch.rand(R, N, 3, generator=gen) * 2 - 1) * draw
    gidx = torch.tensor([0, 1, 1, 0, 5, -2, 1][:R]) if B > 1 else torch.zeros(R, dtype=torch.int64)
    table = torch.randn(B, lay.entries, lay.features_per_level, generator=gen)
    up = torch.randn(R, N, lay.channels, generator=gen)

    p64 = pts.double()
    a = p64.abs().sort(dim=-1, descending=True).values
    q64 = _contract(p64) if contract else p64
    zeroed = torch.zeros(R, N, dtype=torch.bool)
    if contract:
        zeroed |= ((a[..., 0] - 1.0).abs() < KINK_EPS) | ((a[..., 0] > 1.0) & ((a[..., 0] - a[..., 1]) < KINK_EPS))
    for n_l in lay.resolutions:
        x = ((q64 + 1) / 2 * n_l).clamp(-0.5, n_l + 0.5)   # (a coordinate clamped away has no kink)
        zeroed |= ((x - x.round()).abs() < INT_EPS).any(-1)
    left_out = ((q64.abs() - 1.0).abs() < FACE_EPS).any(-1) if mask else torch.zeros(R, N, dtype=torch.bool)
    zeroed |= left_out
    up_live = up * (~zeroed)[..., None]

    p, t64 = p64.clone().requires_grad_(True), table.double().requires_grad_(True)
    want = reference(p, t64, gidx, lay, mask, contract)
    (d_table,) = torch.autograd.grad(want, t64, up.double(), retain_graph=True)
    (touched,) = torch.autograd.grad(want, t64, torch.ones_like(want), retain_graph=True)   # (the weights are >= 0)
    (d_points,) = torch.autograd.grad(want, p, up_live.double())
    inside = (q64.abs() <= 1.0).all(-1) | (not mask)
    _CACHE[name] = dict(lay=lay, pts=pts, gidx=gidx, table=table, up=up, up_live=up_live, mask=mask, contract=contract,
                        zeroed=zeroed, left_out=left_out, inside=inside, want=want.detach(), d_table=d_table, d_points=d_points,
                        untouched=touched == 0)
    return _CACHE[name]


def _encode(c, pts, table, gidx=None):
    return lp.hash_grid_encode(pts, table, c["gidx"].to(pts.device) if gidx is None else gidx, c["lay"],
                               mask_out_of_bounds_samples=c["mask"], contract_coords=c["contract"])


@pytest.mark.parametrize("name", ALL)
def test_values(name):
    dev, c = _dev(), case(name)
    pts, table = c["pts"].to(dev), c["table"].to(dev)
    out = _encode(c, pts, table)
    assert out.shape == c["want"].shape and out.dtype == torch.float32 and out.device == dev
    _worst(f"{name} values", out, c["want"], ~c["left_out"])
    assert torch.equal(_encode(c, pts, table), out), "a second call differs (the forward has no atomics)"
    assert float(out.cpu()[~c["inside"] & ~c["left_out"]].abs().sum()) == 0.0, "a masked point has a feature that is not exactly 0"


@pytest.mark.parametrize("name", ALL)
def test_gradients(name):
    dev, c = _dev(), case(name)
    pts, table = c["pts"].to(dev).requires_grad_(True), c["table"].to(dev).requires_grad_(True)
    out = _encode(c, pts, table)
    (d_table,) = torch.autograd.grad(out, table, c["up"].to(dev), retain_graph=True)
    _worst(f"{name} d table", d_table, c["d_table"])
    assert float(d_table.cpu()[c["untouched"]].abs().sum()) == 0.0, "an entry no point touches is not exactly 0"
    (d_pts,) = torch.autograd.grad(out, pts, c["up_live"].to(dev), retain_graph=True)
    _worst(f"{name} d points", d_pts, c["d_points"])
    assert torch.equal(torch.autograd.grad(out, pts, c["up_live"].to(dev), retain_graph=True)[0], d_pts), "a second point gradient differs"
    gone = ~c["inside"] & ~c["left_out"]
    assert float(d_pts.cpu()[gone].abs().sum()) == 0.0, "a masked point has a gradient"
    (g,) = torch.autograd.grad(out, table, c["up"].to(dev) * gone.to(dev)[..., None])   # the masked points alone
    assert float(g.abs().sum()) == 0.0, "masked points add to the table gradient"


@pytest.mark.parametrize("name", ["mixed", "f8", "masked_contracted"])
@pytest.mark.parametrize("which", ["table", "points"])
def test_only_some_gradients(name, which):
    dev, c = _dev(), case(name)
    pts, table = c["pts"].to(dev).requires_grad_(which == "points"), c["table"].to(dev).requires_grad_(which == "table")
    out = _encode(c, pts, table)
    assert torch.equal(out, _encode(c, pts.detach(), table.detach())), "the forward depends on who asks for a gradient"
    (out * c["up_live"].to(dev)).sum().backward()
    asked, other = (table, pts) if which == "table" else (pts, table)
    assert other.grad is None
    full_p, full_t = c["pts"].to(dev).requires_grad_(True), c["table"].to(dev).requires_grad_(True)
    (_encode(c, full_p, full_t) * c["up_live"].to(dev)).sum().backward()
    if which == "points":
        assert torch.equal(asked.grad, full_p.grad)
    else:
        _worst(f"{name}: d table alone vs with the point gradient", asked.grad, full_t.grad, tol=BAR_ATOMIC)


@pytest.mark.parametrize("shape", [(0, 5), (3, 0)])
def test_empty_batch(shape):
    dev, c = _dev(), case("mixed")
    pts = torch.zeros(shape + (3,), device=dev, requires_grad=True)
    table = c["table"].to(dev).requires_grad_(True)
    out = _encode(c, pts, table, torch.zeros(shape[0], dtype=torch.int64, device=dev))
    assert out.shape == shape + (c["lay"].channels,)
    out.sum().backward()
    assert table.grad.shape == table.shape and float(table.grad.abs().sum()) == 0.0 and pts.grad.shape == pts.shape


def test_graph_capture_forward_and_backward():
    """captured once, replayed on new values: values and the point gradient to the bit, the table gradient (atomics) to BAR_ATOMIC"""
    dev, c = _dev(), case("mixed")
    pts, table = c["pts"].to(dev).requires_grad_(True), c["table"].to(dev).requires_grad_(True)
    up, gidx, static = c["up_live"].to(dev), c["gidx"].to(dev), {}

    def step():
        pts.grad = table.grad = None
        out = _encode(c, pts, table, gidx)
        (out * up).sum().backward()
        static["out"], static["d_pts"], static["d_table"] = out.detach(), pts.grad, table.grad

    _warm_up(step)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    captured = dict(static)
    gen = torch.Generator().manual_seed(79)
    for round_ in range(3):
        if round_:  # new values in the tensors the graph reads
            with torch.no_grad():
                table.copy_(torch.randn(table.shape, generator=gen))
                pts.copy_((torch.rand(pts.shape, generator=gen) * 2 - 1) * 1.2)
        graph.replay()
        torch.cuda.synchronize()
        replayed = {k: v.clone() for k, v in captured.items()}
        step()
        for key in ("out", "d_pts"):
            assert torch.equal(replayed[key], static[key]), f"round {round_}: replayed {key} != eager"
        _worst(f"round {round_}: replayed d table vs eager", replayed["d_table"], static["d_table"], tol=BAR_ATOMIC)
    assert float((static["out"].cpu().double() - c["want"]).abs().max()) > 1e-3  # (the later rounds really saw other values)

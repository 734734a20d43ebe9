"""GPU tests of the total-variation regulariser (lightplane_amd/regularizers.py, csrc/lp_grid_tv.hip).

Reference: the definition in fp64 PyTorch slicing, evaluated on the CPU (`ref_tv`); bar: the project's 1e-4 relative (max |err| /
max |ref| per tensor, tests.test_gpu_parity._assert_close) for the loss and every gradient tensor.  Worst values measured on an
MI355X are recorded in DESIGN.md 4.9."""
import json
import os
import subprocess
import sys

import pytest
import torch

import lightplane_amd as lp
from tests.test_gpu_parity import _assert_close, _rel_err

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MB = 1 << 20


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _phi(d, p):
    return d.abs() if p == 1 else d * d


def ref_tv(grids, p, weights=None):
    """The definition: per grid and per spatial axis of extent > 1 the MEAN of phi(x[i + 1] - x[i]) over all adjacent pairs (all B,
    all C); summed over the axes, weighted over the list.  fp64 in, fp64 out (differentiable)."""
    total = torch.zeros((), dtype=torch.float64)
    for i, g in enumerate(grids):
        assert g.dtype == torch.float64 and g.ndim == 5
        lg = torch.zeros((), dtype=torch.float64)
        for ax in (1, 2, 3):
            n = g.shape[ax]
            if n > 1:
                lg = lg + _phi(g.narrow(ax, 1, n - 1) - g.narrow(ax, 0, n - 1), p).mean()
        total = total + (1.0 if weights is None else float(weights[i])) * lg
    return total


def ref_tv_and_grads(grids32, p, weights=None):
    gs = [g.detach().cpu().double().requires_grad_(True) for g in grids32]
    loss = ref_tv(gs, p, weights)
    if loss.requires_grad and loss.grad_fn is not None:
        loss.backward()
    return loss.detach(), [torch.zeros_like(g) if g.grad is None else g.grad for g in gs]


SHAPES = {
    "voxel": [(2, 9, 7, 5)],
    "triplane": [(2, 1, 7, 5), (2, 9, 1, 5), (2, 9, 7, 1)],
    "mixed": [(2, 9, 7, 5), (2, 1, 7, 5), (2, 9, 1, 5), (2, 9, 7, 1), (2, 1, 1, 5)],
}
WEIGHTS = {"voxel": [0.7], "triplane": [0.5, 2.0, 1.25], "mixed": [1.5, 0.5, 2.0, 1.25, 3.0]}


def _random_grids(shapes, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, C, generator=g) for s in shapes]


@pytest.mark.parametrize("weighted", [False, True], ids=["w1", "wnonuniform"])
@pytest.mark.parametrize("flat", [False, True], ids=["list", "flat"])
@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("C", [1, 3, 16, 32, 64, 128])
@pytest.mark.parametrize("kind", list(SHAPES))
def test_sweep_matches_the_fp64_definition(kind, C, p, flat, weighted):
    dev = _dev()
    host = _random_grids(SHAPES[kind], C, seed=C + p)
    w = WEIGHTS[kind] if weighted else None
    want_loss, want_grads = ref_tv_and_grads(host, p, w)
    if flat:
        x = torch.cat([g.reshape(-1, C) for g in host]).to(dev).requires_grad_(True)
        sizes = [list(g.shape) for g in host]
        loss = lp.grid_tv_loss(x, grid_sizes=sizes, p=p, grid_weights=w)
        loss.backward()
        got = [x.grad]
        want = [torch.cat([g.reshape(-1, C) for g in want_grads])]
        buf = torch.zeros_like(x)
        fused = lp.add_grid_tv_grad_(x.detach(), buf, p=p, grid_sizes=sizes, grid_weights=w)
        bufs = [buf]
    else:
        xs = [g.to(dev).requires_grad_(True) for g in host]
        loss = lp.grid_tv_loss(xs, p=p, grid_weights=w)
        loss.backward()
        got, want = [t.grad for t in xs], want_grads
        bufs = [torch.zeros_like(t) for t in xs]
        fused = lp.add_grid_tv_grad_([t.detach() for t in xs], bufs, p=p, grid_weights=w)
    assert loss.shape == () and loss.dtype == torch.float32 and fused.shape == ()
    errs = {"loss": _rel_err(loss, want_loss), "fused_loss": _rel_err(fused, want_loss)}
    for i, (a, b, r) in enumerate(zip(got, bufs, want)):
        errs[f"grad{i}"] = _rel_err(a, r)
        errs[f"fused_grad{i}"] = _rel_err(b, r)
    print(f"grid_tv {kind} C={C} p={p} flat={flat} weighted={weighted}: worst {max(errs.values()):.2e}")
    _assert_close("loss", loss, want_loss)
    _assert_close("fused loss", fused, want_loss)
    for i, (a, b, r) in enumerate(zip(got, bufs, want)):
        _assert_close(f"grad[{i}]", a, r)
        _assert_close(f"fused grad[{i}]", b, r)


def test_ties_get_an_exactly_zero_gradient():
    """p = 1: inside a constant region every difference is 0 and phi_1'(0) = 0 -- the gradient there is 0.0 bit for bit; a single-cell
    grid has loss 0 and gradient 0."""
    dev = _dev()
    for C in (3, 16):
        x = torch.randn(2, 12, 11, 10, C, generator=torch.Generator().manual_seed(C))
        x[:, 2:9, 3:9, 2:8] = 0.375   # a constant block ...
        x[1, :, :, :, :] = -2.0       # ... and a constant batch entry
        want_loss, want = ref_tv_and_grads([x], 1)
        xd = x.to(dev).requires_grad_(True)
        loss = lp.grid_tv_loss([xd], p=1)
        (loss * 3.0).backward()
        g = xd.grad.cpu()
        inner = g[0, 3:8, 4:8, 3:7].contiguous()
        assert inner.abs().max().item() == 0.0 and (inner.view(torch.int32) & 0x7FFFFFFF).max().item() == 0
        assert (g[1].view(torch.int32) & 0x7FFFFFFF).max().item() == 0
        assert (want[0][0, 3:8, 4:8, 3:7] == 0).all() and (want[0][1] == 0).all()
        _assert_close("loss", loss, want_loss)
        _assert_close("grad", g, 3.0 * want[0])
        buf = torch.full_like(xd, 1.5).detach()
        lp.add_grid_tv_grad_([xd.detach()], [buf], weight=2.0, p=1)
        assert (buf[1] == 1.5).all() and (buf[0, 3:8, 4:8, 3:7] == 1.5).all()   # + 0.0 leaves the buffer as it was
    for p in (1, 2):
        cell = torch.randn(1, 1, 1, 1, 8).to(dev).requires_grad_(True)
        loss = lp.grid_tv_loss([cell], p=p)
        loss.backward()
        assert loss.item() == 0.0 and (cell.grad == 0).all()
        cells = torch.randn(3, 1, 1, 1, 5).to(dev)   # a batch of single cells: no pairs across batch entries
        buf = torch.zeros_like(cells)
        assert lp.add_grid_tv_grad_([cells], [buf], p=p).item() == 0.0 and (buf == 0).all()


def test_no_pairs_across_batch_or_list_entries():
    """A flat tensor whose entries differ wildly in level: a pair across a batch or list boundary would dominate the loss."""
    dev = _dev()
    shapes = [(3, 1, 4, 6), (3, 5, 1, 6), (3, 2, 3, 1)]
    host = []
    for i, s in enumerate(shapes):
        g = torch.randn(*s, 8, generator=torch.Generator().manual_seed(i))
        g += 1000.0 * (i + 1) + 100.0 * torch.arange(3).view(3, 1, 1, 1, 1)
        host.append(g)
    for p in (1, 2):
        want_loss, want = ref_tv_and_grads(host, p)
        x = torch.cat([g.reshape(-1, 8) for g in host]).to(dev).requires_grad_(True)
        loss = lp.grid_tv_loss(x, grid_sizes=[list(g.shape) for g in host], p=p)
        loss.backward()
        # (an fp32 difference of two fp32 values is correctly rounded whatever their level: the bar is the usual one)
        _assert_close("loss", loss, want_loss)
        assert loss.item() < 50.0
        _assert_close("grad", x.grad, torch.cat([g.reshape(-1, 8) for g in want]))


@pytest.mark.parametrize("p", [1, 2])
def test_autograd_upstream_gradient_and_accumulation(p):
    dev = _dev()
    host = _random_grids(SHAPES["mixed"], 16, seed=7)
    w = WEIGHTS["mixed"]
    want_loss, want = ref_tv_and_grads(host, p, w)
    xs = [g.to(dev).requires_grad_(True) for g in host]
    (3.0 * lp.grid_tv_loss(xs, p=p, grid_weights=w)).backward()
    for i, (t, r) in enumerate(zip(xs, want)):
        _assert_close(f"3 x grad[{i}]", t.grad, 3.0 * r)
    # a second backward accumulates into the existing .grad
    (-0.5 * lp.grid_tv_loss(xs, p=p, grid_weights=w)).backward()
    for i, (t, r) in enumerate(zip(xs, want)):
        _assert_close(f"2.5 x grad[{i}]", t.grad, 2.5 * r)
    # composed with other autograd ops, and only some entries requiring a gradient
    ys = [g.to(dev).requires_grad_(i % 2 == 0) for i, g in enumerate(host)]
    loss = lp.grid_tv_loss(ys, p=p, grid_weights=w)
    (loss * loss).backward()
    for i, (t, r) in enumerate(zip(ys, want)):
        if i % 2 == 0:
            _assert_close(f"chain grad[{i}]", t.grad, 2.0 * float(want_loss) * r)
        else:
            assert t.grad is None
    # the fused sweep: same values as the autograd path; adds to (does not overwrite) a non-zero buffer; returns the unweighted loss
    zs = [g.to(dev).requires_grad_(True) for g in host]
    lp.grid_tv_loss(zs, p=p, grid_weights=w).backward()
    zero = [torch.zeros_like(t) for t in zs]
    fused = lp.add_grid_tv_grad_([t.detach() for t in zs], zero, p=p, grid_weights=w)
    _assert_close("fused loss", fused, want_loss)
    for i, (t, b) in enumerate(zip(zs, zero)):
        assert torch.equal(t.grad, b), f"fused gradient {i} differs from the autograd one"
    # (a start of the gradients' own magnitude, ~1e-3: what is added has to show in fp32)
    start = [(1e-3 * torch.randn(t.shape, generator=torch.Generator().manual_seed(i))).to(dev) for i, t in enumerate(zs)]
    bufs = [s.clone() for s in start]
    fused = lp.add_grid_tv_grad_([t.detach() for t in zs], bufs, weight=0.25, p=p, grid_weights=w)
    _assert_close("fused loss (weight 0.25)", fused, want_loss)
    for i, (b, s, r) in enumerate(zip(bufs, start, want)):
        _assert_close(f"accumulated[{i}]", b, s.cpu().double() + 0.25 * r)
        _assert_close(f"added[{i}]", b.cpu().double() - s.cpu().double(), 0.25 * r)
    assert all(not b.requires_grad for b in bufs) and not fused.requires_grad


def test_two_runs_are_bit_identical():
    dev = _dev()
    g = torch.Generator().manual_seed(3)
    host = [torch.randn(2, 40, 33, 37, 32, generator=g), torch.randn(2, 1, 130, 70, 32, generator=g)]
    for p in (1, 2):
        runs = []
        for _ in range(2):
            xs = [t.to(dev).requires_grad_(True) for t in host]
            loss = lp.grid_tv_loss(xs, p=p)
            loss.backward()
            bufs = [torch.ones_like(t) for t in xs]
            fused = lp.add_grid_tv_grad_([t.detach() for t in xs], bufs, weight=0.5, p=p)
            torch.cuda.synchronize()
            runs.append((loss.detach().clone(), [t.grad.clone() for t in xs], fused.clone(), bufs))
        a, b = runs
        assert a[0].view(torch.int32).item() == b[0].view(torch.int32).item() and a[2].view(torch.int32).item() == b[2].view(torch.int32).item()
        assert a[0].view(torch.int32).item() == a[2].view(torch.int32).item()   # the fused sweep reduces in the same order
        for u, v in zip(a[1] + a[3], b[1] + b[3]):
            assert torch.equal(u.view(torch.int32), v.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------------------
# configuration scale
# ------------------------------------------------------------------------------------------------------------------------------


def _fill_random_(x, seed, chunk=1 << 28):
    """x ~ N(0, 1) in place, piecewise (no generator call above 2^31 elements, no full-size temporary)."""
    flat = x.view(-1)
    g = torch.Generator(device=x.device).manual_seed(seed)
    for lo in range(0, flat.numel(), chunk):
        flat[lo:lo + chunk].normal_(generator=g)
    return x


def _host_loss_by_slabs(x, p, slab=16):
    """fp64 loss of ONE grid [B, D, H, W, C] on the device, accumulated slab by slab on the host (a slab = `slab` z-slices plus the
    next one for the pairs along D)."""
    B, D, H, W, C = x.shape
    tot = {1: 0.0, 2: 0.0, 3: 0.0}
    for b in range(B):
        for z0 in range(0, D, slab):
            z1 = min(z0 + slab, D)
            s = x[b, z0:min(z1 + 1, D)].cpu().double()   # [z, H, W, C]
            own = s[: z1 - z0]
            if s.shape[0] > 1:
                tot[1] += _phi(s[1:] - s[:-1], p)[: z1 - z0].sum().item()
            tot[2] += _phi(own[:, 1:] - own[:, :-1], p).sum().item()
            tot[3] += _phi(own[:, :, 1:] - own[:, :, :-1], p).sum().item()
    n = {1: D, 2: H, 3: W}
    cells = B * D * H * W * C
    return sum(tot[a] / (cells // n[a] * (n[a] - 1)) for a in (1, 2, 3) if n[a] > 1)


def _box_reference(x, box, p):
    """fp64 gradient of the TV loss of grid x [1, D, H, W, C] on the cells of `box` = ((z0, z1), (y0, y1), (x0, x1)): the gradient of
    a cell needs its six neighbours only, so the box plus one cell around it (clipped at the grid's faces) goes to the host."""
    _, D, H, W, C = x.shape
    n = (D, H, W)
    lo = [max(b[0] - 1, 0) for b in box]
    hi = [min(b[1] + 1, m) for b, m in zip(box, n)]
    sub = x[0, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]].cpu().double().requires_grad_(True)
    cells = D * H * W * C
    loss = torch.zeros((), dtype=torch.float64)
    for ax in range(3):
        if n[ax] > 1:
            m = sub.shape[ax]
            loss = loss + _phi(sub.narrow(ax, 1, m - 1) - sub.narrow(ax, 0, m - 1), p).sum() / (cells // n[ax] * (n[ax] - 1))
    loss.backward()
    sl = tuple(slice(b[0] - l, b[1] - l) for b, l in zip(box, lo))
    return sub.grad[sl]


def _boxes(D, H, W, k=5):
    """All six faces, two opposite corners and an interior box of a D x H x W grid."""
    mid = lambda n: (n // 2 - k // 2, n // 2 - k // 2 + k)  # noqa: E731
    first, last = (lambda n: (0, k)), (lambda n: (n - k, n))
    out = {"interior": (mid(D), mid(H), mid(W)), "corner000": (first(D), first(H), first(W)), "corner111": (last(D), last(H), last(W))}
    for ax, nm in enumerate("zyx"):
        for end, f in (("0", first), ("1", last)):
            b = [mid(D), mid(H), mid(W)]
            b[ax] = f((D, H, W)[ax])
            out[f"face_{nm}{end}"] = tuple(b)
    return out


def _check_boxes(name, x, grad, p, boxes, scale=1.0):
    worst = 0.0
    for bn, box in boxes.items():
        want = scale * _box_reference(x, box, p)
        got = grad[0, box[0][0]:box[0][1], box[1][0]:box[1][1], box[2][0]:box[2][1]]
        worst = max(worst, _rel_err(got, want))
        _assert_close(f"{name} box {bn}", got, want)
    return worst


@pytest.fixture(scope="module")
def cfg5():
    """The cfg-5 grid, 256^3 x 32 (2.15 GB), and a gradient buffer of its size."""
    dev = _dev()
    x = _fill_random_(torch.empty(1, 256, 256, 256, 32, device=dev), seed=5)
    grad = torch.empty_like(x)
    yield x, grad
    del x, grad
    torch.cuda.empty_cache()


@pytest.mark.parametrize("p", [1, 2])
def test_cfg5_grid_loss_and_gradient_boxes(cfg5, p):
    x, grad = cfg5
    want = _host_loss_by_slabs(x, p)
    boxes = _boxes(256, 256, 256)
    xr = x.detach().requires_grad_(True)
    loss = lp.grid_tv_loss([xr], p=p)
    (2.0 * loss).backward()
    e_loss = _rel_err(loss, want)
    worst = _check_boxes("autograd", x, xr.grad, p, boxes, scale=2.0)
    g_auto = xr.grad
    xr.grad = None
    grad.zero_()   # (an entry is ~1 / (number of pairs) ~ 1e-9: it would vanish in fp32 next to any start value of order 1)
    fused = lp.add_grid_tv_grad_([x], [grad], weight=2.0, p=p)
    e_fused = _rel_err(fused, want)
    worst_f = _check_boxes("fused", x, grad, p, boxes, scale=2.0)
    print(f"grid_tv cfg-5 p={p}: loss err {e_loss:.2e}, fused loss err {e_fused:.2e}, boxes worst {worst:.2e} / fused {worst_f:.2e}")
    _assert_close("loss", loss, want)
    _assert_close("fused loss", fused, want)
    # the whole tensor: the fused sweep adds what the gather backward writes
    assert (grad - g_auto).abs().max().item() <= 1e-6 * g_auto.abs().max().item()


def test_cfg5_memory_is_the_workspace_and_one_gradient(cfg5):
    """What the design allocates, not a measurement: the fused sweep takes the workspace (and a scalar); the autograd path one
    gradient buffer on top."""
    x, grad = cfg5
    ws = lp.grid_tv_workspace_bytes([list(x.shape)])
    grad.zero_()
    lp.add_grid_tv_grad_([x], [grad])   # (first call: library load, kernel images)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = lp.add_grid_tv_grad_([x], [grad], weight=1e-3, p=1)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"grid_tv memory: fused sweep +{rise} bytes (workspace {ws})")
    assert rise <= ws + MB, (rise, ws)
    del loss
    xr = x.detach().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = lp.grid_tv_loss([xr], p=2)
    loss.backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"grid_tv memory: autograd forward + backward +{rise} bytes (gradient {x.numel() * 4}, workspace {ws})")
    assert xr.grad is not None and rise <= x.numel() * 4 + ws + MB, (rise, ws)


def test_grid_above_2_31_elements():
    """512^3 x 32: 2^32 elements (17 GB) -- element offsets are 64-bit.  Boxes past the 2^31-element offset and at the very last rows;
    the loss against the same fp64 definition evaluated slab by slab (on the device: the host pass over 17 GB takes minutes)."""
    dev = _dev()
    n, C = 512, 32
    need = 2 * n ** 3 * C * 4 + (2 << 30)
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info(dev)[0]
    if free < need:
        pytest.skip(f"needs {need / 2**30:.0f} GB of free device memory for the 17 GB grid and its gradient, {free / 2**30:.0f} GB are free")
    x = _fill_random_(torch.empty(1, n, n, n, C, device=dev), seed=9)
    grad = torch.zeros_like(x)
    p = 1
    fused = lp.add_grid_tv_grad_([x], [grad], weight=1.0, p=p)
    k = 5
    boxes = {
        "first_past_2^31": ((n // 2, n // 2 + k), (0, k), (0, k)),           # element 2^31 is cell (z = 256, y = 0, x = 0)
        "straddling_2^31": ((n // 2 - 2, n // 2 + 3), (n - k, n), (n - k, n)),
        "three_quarters": ((3 * n // 4, 3 * n // 4 + k), (n // 2, n // 2 + k), (n // 2, n // 2 + k)),
        "last_rows": ((n - k, n), (n - k, n), (n - k, n)),
        "last_slice_first_rows": ((n - k, n), (0, k), (0, k)),
        "origin": ((0, k), (0, k), (0, k)),
    }
    worst = _check_boxes("17 GB", x, grad, p, boxes)
    tot = [0.0, 0.0, 0.0]
    for z0 in range(0, n, 8):
        s = x[0, z0:min(z0 + 9, n)].double()
        own = s[:8]
        if s.shape[0] > 1:
            tot[0] += _phi(s[1:] - s[:-1], p)[:8].sum().item()
        tot[1] += _phi(own[:, 1:] - own[:, :-1], p).sum().item()
        tot[2] += _phi(own[:, :, 1:] - own[:, :, :-1], p).sum().item()
        del s, own
    want = sum(t / (n ** 3 * C // n * (n - 1)) for t in tot)
    print(f"grid_tv 512^3 x 32: boxes worst {worst:.2e}, loss err {_rel_err(fused, want):.2e}")
    _assert_close("loss", fused, want)
    # the overwrite backward at the same offsets
    xr = x.requires_grad_(True)
    del grad
    lp.grid_tv_loss([xr], p=2).backward()
    _check_boxes("17 GB autograd p=2", x.detach(), xr.grad, 2, boxes)
    xr.grad = None
    del x, xr
    torch.cuda.empty_cache()


def test_graph_capture_of_the_fused_sweep():
    """add_grid_tv_grad_ inside torch.cuda.graph (no host sync, no atomics): two replays reproduce the eager call bit for bit."""
    dev = _dev()
    g = torch.Generator().manual_seed(11)
    xs = [torch.randn(2, 1, 64, 48, 16, generator=g).to(dev), torch.randn(2, 20, 1, 48, 16, generator=g).to(dev),
          torch.randn(2, 20, 64, 1, 16, generator=g).to(dev)]
    w = [0.5, 2.0, 1.25]
    eager = [torch.zeros_like(t) for t in xs]
    eager_loss = lp.add_grid_tv_grad_(xs, eager, weight=0.1, p=1, grid_weights=w).clone()
    bufs = [torch.zeros_like(t) for t in xs]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            lp.add_grid_tv_grad_(xs, bufs, weight=0.1, p=1, grid_weights=w)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = lp.add_grid_tv_grad_(xs, bufs, weight=0.1, p=1, grid_weights=w)
    for _ in range(2):
        for b in bufs:
            b.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss, eager_loss)
        for b, e in zip(bufs, eager):
            assert torch.equal(b, e)
    want_loss, want = ref_tv_and_grads(xs, 1, w)
    _assert_close("replayed loss", loss, want_loss)
    for i, (b, r) in enumerate(zip(bufs, want)):
        _assert_close(f"replayed grad[{i}]", b, 0.1 * r)


def test_fit_synthetic_scene_with_tv_weight():
    """End to end: the example with --tv-weight > 0 runs a few steps in a fresh process with finite losses and gradients."""
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "fit_synthetic_scene.py"), "--steps", "20", "--rays", "2048",
                        "--tv-weight", "0.05"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["tv_weight"] == 0.05 and out["grads_finite"] is True
    for k in ("first_loss", "last_loss", "first_tv", "last_tv", "heldout_psnr_db"):
        assert out[k] == out[k] and abs(out[k]) != float("inf"), (k, out)

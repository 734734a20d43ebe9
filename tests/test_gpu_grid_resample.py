"""GPU tests of the grid-list resampling (lightplane_amd/resample.py, csrc/lp_grid_resample.hip).

Reference: the definition restated in fp64 PyTorch with ``index_select``, axis by axis, on the CPU (`ref_resample`);
bar: the project's 1e-4 relative (max |err| / max |ref| per tensor, tests.test_gpu_parity._assert_close) for every output and every
gradient tensor.  Every case prints its worst value before it asserts."""
import ctypes
import functools
import glob
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib, grids as lp_grids
from tests.test_gpu_parity import _assert_close, _rel_err

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MB = 1 << 20


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


# --------------------------------------------------------------------------------------------------------------------------
# the oracle
# --------------------------------------------------------------------------------------------------------------------------


def _coeff(n_in, n_out, align, scale):
    """the ONE fp32 host coefficient of an axis"""
    if align:
        return np.float32(0.0) if n_out == 1 else np.float32(n_in - 1) / np.float32(n_out - 1)
    if scale is not None:
        return np.float32(1.0 / scale)
    return np.float32(n_in) / np.float32(n_out)


def ref_resample(x, out_dhw, align, scale=None):
    """The definition on one fp64 grid ``[B, D, H, W, C]``: per spatial axis src(o), i0, i1, lambda, then the two-row blend; the three
    axes one after the other (the tensor product).  Differentiable."""
    assert x.dtype == torch.float64 and x.ndim == 5
    y = x
    for ax in range(3):
        n_in, n_out = x.shape[1 + ax], int(out_dhw[ax])
        a = float(_coeff(n_in, n_out, align, scale))
        o = torch.arange(n_out, dtype=torch.float64)
        src = a * o if align else (a * (o + 0.5) - 0.5).clamp_min(0.0)
        i0 = src.floor().long().clamp_max(n_in - 1)
        i1 = (i0 + 1).clamp_max(n_in - 1)
        lam = (src - i0.double()).clamp(0.0, 1.0)
        shape = [1] * 5
        shape[1 + ax] = n_out
        y = y.index_select(1 + ax, i0) * (1.0 - lam).view(shape) + y.index_select(1 + ax, i1) * lam.view(shape)
    return y


SHAPES = {
    "voxel_2x5x4x3": [(2, 5, 4, 3)],
    "voxel_1x9x7x5": [(1, 9, 7, 5)],
    "plane_xy": [(2, 1, 7, 5)],
    "plane_xz": [(2, 9, 1, 5)],
    "plane_yz": [(2, 9, 7, 1)],
    "mixed": [(2, 9, 7, 5), (2, 1, 7, 5), (2, 9, 1, 5), (2, 9, 7, 1), (2, 1, 1, 5)],
}
MAPPINGS = ("factor2", "factor1p5", "sizes_plus3", "down_half_plus1")


def _targets(shapes, mapping):
    """(per-grid [D', H', W'], scale factor or None); a singular axis stays singular in every mapping"""
    if mapping.startswith("factor"):
        f = {"factor2": 2.0, "factor1p5": 1.5}[mapping]
        return [[n if n == 1 else int(math.floor(n * f)) for n in s[1:]] for s in shapes], f
    if mapping == "sizes_plus3":
        return [[n if n == 1 else n + 3 for n in s[1:]] for s in shapes], None
    return [[n // 2 + 1 for n in s[1:]] for s in shapes], None


@functools.lru_cache(maxsize=None)
def _case(shape_key, C, align, mapping):
    """inputs, upstream gradients and the oracle's outputs and gradients of one case: computed once, shared by both containers, never
    modified (CPU tensors)"""
    shapes = SHAPES[shape_key]
    out_dhw, scale = _targets(shapes, mapping)
    gen = torch.Generator().manual_seed(1000 * C + 10 * MAPPINGS.index(mapping) + int(align))
    xs = [torch.randn(*s, C, generator=gen) for s in shapes]
    gys = [torch.randn(s[0], *o, C, generator=gen) for s, o in zip(shapes, out_dhw)]
    ref_y, ref_gx = [], []
    for x, gy, o in zip(xs, gys, out_dhw):
        x64 = x.double().requires_grad_(True)
        y = ref_resample(x64, o, align, scale)
        ref_y.append(y.detach())
        ref_gx.append(torch.autograd.grad(y, x64, gy.double())[0])
    return xs, gys, out_dhw, scale, ref_y, ref_gx


def _run(xs, gys, out_dhw, scale, align, flat):
    """forward and autograd backward on the GPU; returns (outputs, input gradients) as lists of 5-D tensors"""
    dev = _dev()
    kw = dict(scale_factor=scale) if scale is not None else dict(sizes=out_dhw)
    if not flat:
        gx = [x.to(dev).requires_grad_(True) for x in xs]
        ys = lp.grid_resample(gx, align_corners=align, **kw)
        assert isinstance(ys, list) and len(ys) == len(xs)
        grads = torch.autograd.grad(ys, gx, [g.to(dev) for g in gys])
        return ys, list(grads)
    C = xs[0].shape[-1]
    sizes = [list(x.shape) for x in xs]
    fx = torch.cat([x.reshape(-1, C) for x in xs]).to(dev).requires_grad_(True)
    fy, new_sizes = lp.grid_resample(fx, sizes, align_corners=align, **kw)
    assert new_sizes == [[x.shape[0]] + list(o) + [C] for x, o in zip(xs, out_dhw)]
    assert fy.shape == (sum(s[0] * s[1] * s[2] * s[3] for s in new_sizes), C)
    fg, = torch.autograd.grad(fy, fx, torch.cat([g.reshape(-1, C) for g in gys]).to(dev))
    return list(lp_grids.unflatten_grid(fy, new_sizes)), list(lp_grids.unflatten_grid(fg, sizes))


@pytest.mark.parametrize("flat", [False, True], ids=["list", "flat"])
@pytest.mark.parametrize("mapping", MAPPINGS)
@pytest.mark.parametrize("align", [False, True], ids=["nac", "ac"])
@pytest.mark.parametrize("C", [1, 3, 16, 32, 64, 128])
@pytest.mark.parametrize("shape_key", list(SHAPES))
def test_forward_and_adjoint_match_the_definition(shape_key, C, align, mapping, flat):
    xs, gys, out_dhw, scale, ref_y, ref_gx = _case(shape_key, C, align, mapping)
    ys, gxs = _run(xs, gys, out_dhw, scale, align, flat)
    worst_y = max(_rel_err(y, r) for y, r in zip(ys, ref_y))
    worst_g = max(_rel_err(g, r) for g, r in zip(gxs, ref_gx))
    print(f"resample {shape_key} C={C} align={align} {mapping} {'flat' if flat else 'list'}: forward {worst_y:.3e}  adjoint {worst_g:.3e}")
    for k, (y, r) in enumerate(zip(ys, ref_y)):
        assert tuple(y.shape) == tuple(r.shape)
        _assert_close(f"out[{k}]", y, r)
    for k, (g, r) in enumerate(zip(gxs, ref_gx)):
        _assert_close(f"grad[{k}]", g, r)


def test_a_singular_axis_replicates_when_it_is_given_an_extent():
    """explicit sizes may grow an axis of extent 1: every output cell along it is the one input cell"""
    dev = _dev()
    x = torch.randn(2, 1, 3, 4, 8, generator=torch.Generator().manual_seed(3))
    for align in (False, True):
        y, = lp.grid_resample([x.to(dev)], sizes=[3, 5, 4], align_corners=align)
        ref = ref_resample(x.double(), [3, 5, 4], align)
        print(f"replicate align={align}: {_rel_err(y, ref):.3e}")
        _assert_close("replicated", y, ref)
        _assert_close("slices", y[:, 2], y[:, 0].cpu(), tol=1e-6)


# --------------------------------------------------------------------------------------------------------------------------
# adjoint identity, accumulate, reproducibility
# --------------------------------------------------------------------------------------------------------------------------


def _abi_backward(grads, g_outs, align, scale, accumulate):
    """lp_grid_resample_backward on lists of 5-D GPU tensors"""
    C = grads[0].shape[-1]

    def as_list(ts):
        descs = [lp_grids.GridDesc(*t.shape[:4], 0) for t in ts]
        return _lib.make_grid_list([t.view(-1, C) for t in ts], descs, C, 0)

    src, dst = as_list(grads), as_list(g_outs)
    co = None
    if scale is not None and not align:
        co = (ctypes.c_float * (3 * len(grads)))(*([1.0 / scale] * (3 * len(grads))))
    rc = _lib.lib().lp_grid_resample_backward(ctypes.byref(src), ctypes.byref(dst), int(align), co, int(accumulate),
                                              _lib.current_stream(grads[0].device))
    _lib.check(rc, "lp_grid_resample_backward")


@pytest.mark.parametrize("shape_key,mapping,align", [("voxel_1x9x7x5", "factor1p5", False), ("mixed", "factor2", True),
                                                     ("voxel_2x5x4x3", "down_half_plus1", False)],
                         ids=["voxel", "triplane_and_more", "downsampling"])
def test_adjoint_identity_and_accumulate(shape_key, mapping, align):
    """<R x, y> == <x, R^T y> in fp64 from the GPU's fp32 results, to 1e-5 relative; the accumulate variant adds exactly R^T y"""
    dev = _dev()
    xs, gys, out_dhw, scale, _, _ = _case(shape_key, 32, align, mapping)
    kw = dict(scale_factor=scale) if scale is not None else dict(sizes=out_dhw)
    gx = [x.to(dev).requires_grad_(True) for x in xs]
    ys = lp.grid_resample(gx, align_corners=align, **kw)
    gy = [g.to(dev) for g in gys]
    rty = torch.autograd.grad(ys, gx, gy)
    lhs = sum((y.detach().double() * g.double()).sum() for y, g in zip(ys, gy)).item()
    rhs = sum((x.detach().double() * r.double()).sum() for x, r in zip(gx, rty)).item()
    rel = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
    print(f"adjoint identity {shape_key} {mapping} align={align}: <Rx, y> = {lhs:.9e}  <x, RTy> = {rhs:.9e}  rel {rel:.3e}")
    assert rel <= 1e-5
    # accumulate onto a non-zero buffer: one fp32 addition per element on top of the same sum
    gen = torch.Generator().manual_seed(7)
    buf0 = [torch.randn(*x.shape, generator=gen).to(dev) for x in xs]
    buf = [b.clone() for b in buf0]
    _abi_backward(buf, gy, align, scale, accumulate=1)
    for b, b0, r in zip(buf, buf0, rty):
        assert torch.equal(b, b0 + r)
    # ... and the overwrite variant ignores what the buffer held
    _abi_backward(buf, gy, align, scale, accumulate=0)
    for b, r in zip(buf, rty):
        assert torch.equal(b, r)


def test_forward_and_backward_are_bit_reproducible():
    dev = _dev()
    xs, gys, out_dhw, scale, _, _ = _case("mixed", 32, False, "factor1p5")
    res = []
    for _ in range(2):
        gx = [x.to(dev).requires_grad_(True) for x in xs]
        ys = lp.grid_resample(gx, scale_factor=scale)
        res.append((ys, torch.autograd.grad(ys, gx, [g.to(dev) for g in gys])))
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b)
    for a, b in zip(res[0][1], res[1][1]):
        assert torch.equal(a, b)


# --------------------------------------------------------------------------------------------------------------------------
# tiles, alignment
# --------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("align", [False, True], ids=["nac", "ac"])
def test_upsample_across_tile_boundaries(align):
    """(1, 33, 17, 20) x 32 by 2: many workgroups per slice, output rows of 40 * 8 = 320 lane positions (no multiple of the 256-lane
    tile: tiles straddle rows and end mid-slice); (1, 3, 5, 32) x 32: rows of 64 * 8 = 512 (two whole tiles)."""
    dev = _dev()
    gen = torch.Generator().manual_seed(11)
    shapes = [(1, 33, 17, 20), (1, 3, 5, 32)]
    xs = [torch.randn(*s, 32, generator=gen) for s in shapes]
    gx = [x.to(dev).requires_grad_(True) for x in xs]
    ys = lp.grid_resample(gx, scale_factor=2.0, align_corners=align)
    assert [tuple(y.shape) for y in ys] == [(1, 66, 34, 40, 32), (1, 6, 10, 64, 32)]
    gys = [torch.randn(*y.shape, generator=gen) for y in ys]
    grads = torch.autograd.grad(ys, gx, [g.to(dev) for g in gys])
    for k, (x, gy, y, g) in enumerate(zip(xs, gys, ys, grads)):
        x64 = x.double().requires_grad_(True)
        ref = ref_resample(x64, y.shape[1:4], align, 2.0)
        ref_g, = torch.autograd.grad(ref, x64, gy.double())
        print(f"tiles align={align} grid {k}: forward {_rel_err(y, ref.detach()):.3e}  adjoint {_rel_err(g, ref_g):.3e}")
        _assert_close(f"out[{k}]", y, ref.detach())
        _assert_close(f"grad[{k}]", g, ref_g)


def test_under_aligned_views_take_the_scalar_path_bit_for_bit():
    """a dense view 4 bytes into a buffer (C = 4: the 16-byte path would apply) is read float by float, not copied, and gives the
    aligned tensor's result exactly -- forward and backward, and as the gradient's destination through the C ABI"""
    dev = _dev()
    shape = (2, 5, 4, 3, 4)
    n = math.prod(shape)
    gen = torch.Generator().manual_seed(5)
    buf = torch.randn(n + 1, generator=gen).to(dev)
    view = buf[1:].view(shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    aligned = view.clone()
    assert aligned.data_ptr() % 16 == 0
    outs = []
    for x in (view, aligned):
        x = x.detach().requires_grad_(True)
        y, = lp.grid_resample([x], scale_factor=1.5)
        gy = torch.randn(*y.shape, generator=torch.Generator().manual_seed(6)).to(dev)
        outs.append((y, torch.autograd.grad(y, x, gy)[0], gy))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    ref = ref_resample(aligned.cpu().double(), outs[1][0].shape[1:4], False, 1.5)
    _assert_close("aligned result", outs[1][0], ref)
    gbuf = torch.zeros(n + 1, device=dev)
    _abi_backward([gbuf[1:].view(shape)], [outs[1][2]], False, 1.5, accumulate=0)
    assert torch.equal(gbuf[1:].view(shape), outs[1][1]) and float(gbuf[0]) == 0.0


# --------------------------------------------------------------------------------------------------------------------------
# grid_up_sample against the reference's helper
# --------------------------------------------------------------------------------------------------------------------------

GOLDEN = sorted(glob.glob(os.path.join(REPO, "tests", "golden", "gridop_upsample_*.npz")))


def test_golden_files_are_all_there():
    names = {os.path.basename(p) for p in GOLDEN}
    want = {f"gridop_upsample_{k}_f{f}_{a}.npz" for k in ("voxel", "triplane") for f in ("2p0", "1p5") for a in ("nac", "ac")}
    assert names == want
    assert all(os.path.getsize(p) < 100 * 1024 for p in GOLDEN)


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[len("gridop_upsample_"):-4] for p in GOLDEN])
def test_grid_up_sample_matches_the_reference_helper(path):
    dev = _dev()
    z = np.load(path)
    n = sum(1 for k in z.files if k.startswith("in_"))
    ins = [torch.from_numpy(z[f"in_{k}"]).to(dev).requires_grad_(True) for k in range(n)]
    grids = list(ins)
    ret = lp.grid_up_sample(grids, upsample_factor=float(z["factor"]), align_corners=bool(z["align_corners"]))
    assert ret is grids and len(grids) == n
    for k in range(n):
        want = z[f"out_{k}"]
        g = grids[k]
        assert g is not ins[k] and tuple(g.shape) == want.shape
        assert g.is_leaf and g.requires_grad and g.grad_fn is None and g.is_contiguous()
        for ax in (1, 2, 3):
            assert (g.shape[ax] == 1) == (ins[k].shape[ax] == 1)  # a plane stays a plane
        print(f"grid_up_sample {os.path.basename(path)} grid {k}: {_rel_err(g, want):.3e}")
        _assert_close(f"grid[{k}]", g, want)


# --------------------------------------------------------------------------------------------------------------------------
# memory, graph capture, example
# --------------------------------------------------------------------------------------------------------------------------


def test_forward_allocates_its_result_only():
    """(1, 64, 64, 64, 32) by 2: the 268 MB result and nothing else -- a derived bound (the op allocates its result only) plus 1 MB
    of allocator rounding"""
    dev = _dev()
    x = torch.randn(1, 64, 64, 64, 32, device=dev)
    out_bytes = 128 ** 3 * 32 * 4
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.max_memory_allocated(dev)
    with torch.no_grad():
        y, = lp.grid_resample([x], scale_factor=2.0)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(dev) - before
    print(f"memory: result {out_bytes / MB:.1f} MB, peak rise {rise / MB:.1f} MB")
    assert tuple(y.shape) == (1, 128, 128, 128, 32)
    assert rise <= out_bytes + MB
    # (and the values: the 8 cells of an interior 2 x 2 x 2 output block blend the same 8 input cells)
    ref = ref_resample(x[:, :3, :3, :3].cpu().double(), [6, 6, 6], False, 2.0)
    _assert_close("corner block", y[:, :4, :4, :4], ref[:, :4, :4, :4])


def test_graph_capture_of_forward_and_backward():
    """forward + backward capture into one graph (no host synchronisation, no allocation by the library, launches on the capturing
    stream; a single chain of kernels) and the replay reproduces the eager values on new inputs"""
    dev = _dev()
    xs, gys, out_dhw, scale, _, _ = _case("mixed", 16, False, "factor2")
    static_x = [x.to(dev).requires_grad_(True) for x in xs]
    static_gy = [g.to(dev) for g in gys]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up on the side stream, as torch.cuda.graph asks for
        ys = lp.grid_resample(static_x, scale_factor=scale)
        torch.autograd.grad(ys, static_x, static_gy)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_y = lp.grid_resample(static_x, scale_factor=scale)
        static_g = torch.autograd.grad(static_y, static_x, static_gy)
    gen = torch.Generator().manual_seed(99)
    new_x = [torch.randn(*x.shape, generator=gen) for x in xs]
    new_gy = [torch.randn(*g.shape, generator=gen) for g in gys]
    with torch.no_grad():
        for t, v in zip(static_x, new_x):
            t.copy_(v)
        for t, v in zip(static_gy, new_gy):
            t.copy_(v)
    graph.replay()
    torch.cuda.synchronize()
    eager_x = [v.to(dev).requires_grad_(True) for v in new_x]
    eager_y = lp.grid_resample(eager_x, scale_factor=scale)
    eager_g = torch.autograd.grad(eager_y, eager_x, [v.to(dev) for v in new_gy])
    for a, b in zip(static_y, eager_y):
        assert torch.equal(a, b)
    for a, b in zip(static_g, eager_g):
        assert torch.equal(a, b)


def test_fit_synthetic_scene_coarse_to_fine():
    """the example with an upsampling schedule: planes end at the final resolution, and the fit goes on improving after the first
    upsampling"""
    spec = importlib.util.spec_from_file_location("fit_synthetic_scene", os.path.join(REPO, "examples", "fit_synthetic_scene.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    old = lp.config.stop_transmittance
    try:
        r = mod.fit(steps=60, n_rays=2048, res=32, upsample_steps=(20, 40))
    finally:
        lp.config.stop_transmittance = old
    print("coarse-to-fine fit:", r)
    assert r["upsample_steps"] == [20, 40] and r["start_res"] == 8
    assert r["grid_shapes"] == [[1, 1, 32, 32, 16], [1, 32, 1, 32, 16], [1, 32, 32, 1, 16]]
    assert math.isfinite(r["heldout_psnr_db"]) and math.isfinite(r["psnr_at_upsample_db"][0])
    assert r["heldout_psnr_db"] > r["psnr_at_upsample_db"][0], r

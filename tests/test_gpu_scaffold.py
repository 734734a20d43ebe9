"""The fused occupancy scaffold (lightplane_amd/scaffold.py, csrc/lp_scaffold.hip) against its fp64 definition.

Oracle: ``oracle.lightplane_oracle.eval_decoder`` in fp64 on the explicit lattice ``linspace(0, 1, n) * 2 - 1`` (built as
tests/test_gpu_parity.py::test_module_point_evaluation_and_scaffold builds it), followed by ``max_pool3d`` and ``> t`` on the CPU.
* the opacity lattice is held to the project's bar: max |err| / max |ref| <= 1e-4;
* the occupancy is held to EXACT equality at a threshold the oracle alone proves unambiguous: the midpoint of the widest gap between
  consecutive sorted oracle opacities inside their 30-70 % quantile range, and that gap has to exceed 2e-4 * max |opacity| -- twice the
  kernel's allowance, so no lattice point can sit on the wrong side.  The condition is on the inputs (``test_thresholds_are_unambiguous``
  checks it without a GPU kernel in the loop): a seed that fails it is changed, never the bar.
"""
import importlib.util
import math
import os

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import config
from oracle import lightplane_oracle as O
from tests.layouts import make_layout
from tests.synth import grid_sizes_for, random_decoder
from tests.test_gpu_parity import _assert_close, _dev, _rel_err

pytestmark = pytest.mark.gpu

GAP = 2e-4  # least relative gap around an occupancy threshold: twice the opacity bar


def _grid_sizes(kind, base):
    if kind == "voxel":
        return grid_sizes_for(base, False)
    if kind == "triplane":
        return grid_sizes_for(base, True)
    assert kind == "mixed", kind  # a voxel grid and an xz plane of another resolution
    B, D, H, W, C = base
    return [list(base), [B, D + 2, 1, W + 3, C]]


#   name: scaffold [B, D, H, W], grid kind, grid base [B, D, H, W, C], (trunk layers, opacity layers, hidden), dilate, mask, grid form
CASES = {
    "triplane_c16_22x32_r1": ((2, 6, 5, 7), "triplane", (2, 6, 5, 7, 16), (2, 2, 32), 1, False, "list"),
    "voxel_c32_11x64_r3_wide": ((1, 3, 2, 70), "voxel", (1, 4, 3, 5, 32), (1, 1, 64), 3, True, "list"),
    "mixed_c16_22x32_point": ((1, 1, 1, 1), "mixed", (1, 3, 4, 5, 16), (2, 2, 32), 1, False, "list"),
    "mixed_c64_44x64_r0_flat": ((2, 9, 1, 5), "mixed", (2, 3, 4, 5, 64), (4, 4, 64), 0, False, "flat"),
    "voxel_c32_twogrid_r3_flat": ((2, 6, 5, 7), "voxel", (2, 5, 4, 6, 32), (0, 2, 32), 3, False, "flat"),
    "triplane_c64_twogrid_1layer_r1": ((1, 3, 2, 70), "triplane", (1, 8, 7, 9, 64), (0, 1, 64), 1, True, "list"),
    "triplane_c16_44x64_r3": ((2, 9, 1, 5), "triplane", (2, 6, 5, 7, 16), (4, 4, 64), 3, True, "list"),
    "mixed_c32_11x64_r0_flat": ((2, 6, 5, 7), "mixed", (2, 3, 4, 5, 32), (1, 1, 64), 0, True, "flat"),
    "voxel_c16_22x128_r1": ((1, 3, 2, 70), "voxel", (1, 4, 3, 5, 16), (2, 2, 128), 1, False, "list"),  # the widest layers: 64 KB of LDS
    # ragged widths (tests/ragged_cases.py; the names sort after every other one: the seeds of the rows above depend on the sorted order)
    "width7_voxel_c5_22_r1": ((2, 6, 5, 7), "voxel", (2, 4, 3, 5, 5), (2, 2, 7), 1, True, "list"),
    "width33_triplane_c20_22_r3": ((1, 3, 2, 70), "triplane", (1, 6, 5, 7, 20), (2, 2, 33), 3, False, "flat"),
}
GAIN = 1.7
_CACHE = {}


def _decoder(gen, n_t, n_o, C, hidden):
    return random_decoder(gen, n_t, n_o, 2, C, hidden, 3, use_separate_color_grid=(n_t == 0), std=(2.0 / hidden) ** 0.5)


def _lattice(D, H, W):
    lin = lambda n: torch.linspace(0, 1, n) * 2 - 1  # noqa: E731
    zz, yy, xx = torch.meshgrid(lin(D), lin(H), lin(W), indexing="ij")
    return torch.stack([xx, yy, zz], -1).reshape(1, -1, 3)


def oracle_opacity(grids, dec, size, gain, mask=False):
    """fp64 opacity [B, D, H, W] of the decoder on the scaffold's lattice"""
    B, D, H, W = size
    g64 = [g.double() for g in grids]
    d64 = lp.DecoderParams(dec.mlp_params.detach().cpu().double(), dec.n_hidden_trunk.cpu(), dec.n_hidden_opacity.cpu(),
                           dec.n_hidden_color.cpu(), dec.color_chn)
    enc = torch.zeros(1, int(dec.n_hidden_color[0]), dtype=torch.float64)
    pts = _lattice(D, H, W).double()
    return torch.stack([O.eval_decoder(pts, g64, torch.tensor([b]), d64, enc, gain, mask_out_of_bounds_samples=mask)[0].reshape(D, H, W)
                        for b in range(B)])


def unambiguous_threshold(op64, q_lo=0.3, q_hi=0.7):
    """(t, relative gap): the midpoint of the widest gap between consecutive sorted values inside the 30-70 % quantile range.  A
    lattice of fewer than 4 points has no such range: half its smallest value (the gap is then that value itself)."""
    v = op64.flatten().sort().values
    n, top = v.numel(), float(op64.abs().max())
    if n < 4:
        return 0.5 * float(v[0]), 0.5 * float(v[0]) / top
    lo, hi = int(q_lo * n), max(int(q_hi * n), int(q_lo * n) + 1)
    gaps = v[lo + 1: hi + 1] - v[lo: hi]
    k = int(gaps.argmax())
    return 0.5 * float(v[lo + k] + v[lo + k + 1]), float(gaps[k]) / top


def oracle_occupancy(op64, t, r):
    if r > 0:
        op64 = torch.nn.functional.max_pool3d(op64, kernel_size=2 * r + 1, padding=r, stride=1)
    return (op64 > t).float()


def _case(name):
    """inputs and oracle of a case, computed once and never modified"""
    if name not in _CACHE:
        size, kind, base, (n_t, n_o, hidden), r, mask, form = CASES[name]
        gen = torch.Generator().manual_seed(sorted(CASES).index(name) + 100)
        grids = [0.5 * torch.randn(s, generator=gen) for s in _grid_sizes(kind, base)]
        dec = _decoder(gen, n_t, n_o, base[4], hidden)
        op = oracle_opacity(grids, dec, size, GAIN, mask)
        t, gap = unambiguous_threshold(op)
        _CACHE[name] = dict(size=list(size), grids=grids, dec=dec, op=op, t=t, gap=gap, r=r, mask=mask, form=form)
    return _CACHE[name]


def _on(dev, c):
    """(grid argument, grid_sizes, decoder) of a case on the GPU, in the case's grid form"""
    dec = c["dec"]
    ddec = lp.DecoderParams(dec.mlp_params.to(dev), dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
    if c["form"] == "flat":
        C = c["grids"][0].shape[-1]
        return torch.cat([g.reshape(-1, C) for g in c["grids"]]).to(dev), [list(g.shape) for g in c["grids"]], ddec
    return [g.to(dev) for g in c["grids"]], None, ddec


@pytest.mark.parametrize("name", list(CASES))
def test_thresholds_are_unambiguous(name):
    """the condition on the inputs, from the oracle alone"""
    c = _case(name)
    print(f"{name}: threshold {c['t']:.6g}, gap {c['gap']:.3e} of max |opacity| {float(c['op'].abs().max()):.4g}")
    assert c["gap"] > GAP, f"{name}: widest gap {c['gap']:.3e} <= {GAP}: change the seed"
    assert 0 < float((c["op"] > c["t"]).float().mean()) < 1 or c["op"].numel() < 4


@pytest.mark.parametrize("name", list(CASES))
def test_opacity_lattice(name):
    dev, c = _dev(), _case(name)
    grid, sizes, dec = _on(dev, c)
    got = lp.scaffold_opacity(grid, dec, c["size"], gain=GAIN, mask_out_of_bounds_samples=c["mask"], grid_sizes=sizes)
    assert got.shape == tuple(c["size"]) and got.dtype == torch.float32 and got.device == dev
    print(f"{name}: worst |err| / max |ref| = {_rel_err(got, c['op'].numpy()):.3e}")
    _assert_close(f"opacity lattice {name}", got, c["op"].numpy(), tol=1e-4)


@pytest.mark.parametrize("name", list(CASES))
def test_occupancy_is_exact(name):
    dev, c = _dev(), _case(name)
    assert c["gap"] > GAP
    grid, sizes, dec = _on(dev, c)
    for r in sorted({c["r"], 0}):
        want = oracle_occupancy(c["op"], c["t"], r)
        got = lp.calculate_scaffold(grid, dec, c["size"], gain=GAIN, threshold=c["t"], dilate_scaffold=r,
                                    mask_out_of_bounds_samples=c["mask"], grid_sizes=sizes)
        assert got.shape == tuple(c["size"]) and got.dtype == torch.float32
        assert set(got.unique().tolist()) <= {0.0, 1.0}
        bad = int((got.cpu() != want).sum())
        assert bad == 0, f"{name}, dilate {r}: {bad} of {want.numel()} lattice points differ from the oracle"
    if c["size"][0] == 2:  # different content per batch element: different scaffolds
        want0 = oracle_occupancy(c["op"], c["t"], 0)
        assert not torch.equal(want0[0], want0[1])
        got0 = lp.calculate_scaffold(grid, dec, c["size"], gain=GAIN, threshold=c["t"], dilate_scaffold=0,
                                     mask_out_of_bounds_samples=c["mask"], grid_sizes=sizes)
        assert not torch.equal(got0[0], got0[1])


def test_every_dilation_radius_on_one_lattice():
    """r in {0, 1, 3} and a window wider than every axis, on the lattice whose W crosses a 64-lane boundary and whose H is smaller than
    the radius"""
    dev, c = _dev(), _case("voxel_c32_11x64_r3_wide")
    grid, sizes, dec = _on(dev, c)
    for r in (0, 1, 3, 70, 1000):
        got = lp.calculate_scaffold(grid, dec, c["size"], gain=GAIN, threshold=c["t"], dilate_scaffold=r,
                                    mask_out_of_bounds_samples=c["mask"], grid_sizes=sizes)
        assert torch.equal(got.cpu(), oracle_occupancy(c["op"], c["t"], r)), f"dilate {r}"
    assert float(got.min()) == 1.0  # (the last window covers everything and something is occupied)


def test_default_threshold_gives_all_ones():
    dev, c = _dev(), _case("triplane_c16_22x32_r1")
    assert float(c["op"].min()) > 1e-5  # every opacity of this decoder is far above the default threshold 1e-7
    grid, sizes, dec = _on(dev, c)
    got = lp.calculate_scaffold(grid, dec, c["size"], gain=GAIN)
    assert got.shape == tuple(c["size"]) and float(got.min()) == 1.0 and float(got.max()) == 1.0


def test_underflowing_softplus_gives_all_zeros():
    """opacity_init_bias = -200: softplus(raw) is 1e-87 in fp64 and underflows to exactly 0 in fp32 -- both below the threshold"""
    dev = _dev()
    dec = lp.init_decoder_params(device="cpu", n_layers_opacity=2, n_layers_trunk=2, n_layers_color=2, input_chn=16, hidden_chn=32,
                                 color_chn=3, opacity_init_bias=-200.0)
    gen = torch.Generator().manual_seed(3)
    grids = [0.5 * torch.randn(s, generator=gen) for s in grid_sizes_for((2, 6, 5, 7, 16), True)]
    size = [2, 6, 5, 7]
    op = oracle_opacity(grids, dec, size, 1.0)
    assert 0.0 < float(op.max()) < 1e-30
    ddec = lp.DecoderParams(dec.mlp_params.to(dev), dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
    for r in (0, 2):
        got = lp.calculate_scaffold([g.to(dev) for g in grids], ddec, size, dilate_scaffold=r)
        assert float(got.max()) == 0.0 and got.shape == tuple(size)
    assert float(lp.scaffold_opacity([g.to(dev) for g in grids], ddec, size).max()) < 1e-30


def test_grid_layouts_at_the_boundary():
    """The grid goes to the kernels as it is: a dense view at a 16-byte aligned offset into a larger buffer is read in place and gives the
    same bits; a non-contiguous entry is refused by the front-end, an under-aligned one by the library -- neither is copied."""
    dev, c = _dev(), _case("triplane_c16_22x32_r1")
    grid, _, dec = _on(dev, c)
    want = lp.scaffold_opacity(grid, dec, c["size"], gain=GAIN)
    n = grid[1].numel()
    buf = torch.randn(n + 8, device=dev)
    view = buf[4: 4 + n].view(grid[1].shape)
    view.copy_(grid[1])
    assert view.data_ptr() % 16 == 0 and view.data_ptr() != buf.data_ptr()
    assert torch.equal(lp.scaffold_opacity([grid[0], view, grid[2]], dec, c["size"], gain=GAIN), want)
    _, strided = make_layout(c["grids"][1], "strided", kind="grid").on(dev)
    assert not strided.is_contiguous() and torch.equal(strided, grid[1])
    for fn in (lp.scaffold_opacity, lp.calculate_scaffold):
        with pytest.raises(AssertionError, match="contiguous"):
            fn([grid[0], strided, grid[2]], dec, c["size"], gain=GAIN)
        for variant in ("off4", "off8"):
            _, off = make_layout(c["grids"][1], variant).on(dev)
            assert off.is_contiguous() and off.data_ptr() % 16 != 0
            with pytest.raises(AssertionError, match="16-byte aligned"):
                fn([grid[0], off, grid[2]], dec, c["size"], gain=GAIN)


def _module(dev, two_grid=False):
    torch.manual_seed(0)
    mod = lp.LightplaneRenderer(num_samples=8, color_chn=3, grid_chn=16, mlp_hidden_chn=32, gain=2.0, opacity_init_bias=-1.0,
                                ray_embedding_num_harmonics=None, use_separate_color_grid=two_grid).to(dev)
    with torch.no_grad():  # (a spread of opacities around the threshold; the two-grid decoder has no trunk to damp the factor)
        mod.mlp_params.mul_(1.5 if two_grid else 3.0)
    return mod


@pytest.mark.parametrize("two_grid", [False, True])
def test_module_calls_the_fused_function(two_grid):
    """config.fused_module_ops on: LightplaneRenderer.calculate_scaffold IS the functional call (the module's gain and mask), bit for bit;
    off: the Renderer path gives the same scaffold at a threshold no lattice point is near."""
    dev = _dev()
    mod = _module(dev, two_grid)
    gen = torch.Generator().manual_seed(7)
    grids = [0.5 * torch.randn(s, generator=gen) for s in grid_sizes_for((2, 6, 5, 7, 16), True)]
    dgrids = [g.to(dev) for g in grids]
    size = [2, 6, 5, 7]
    op = oracle_opacity(grids, mod.get_decoder_params(), size, 2.0)
    t, gap = unambiguous_threshold(op)
    assert gap > GAP, f"gap {gap:.3e}: change the seed"
    assert config.fused_module_ops
    for r in (0, 1, 2):
        got = mod.calculate_scaffold(dgrids, size, dev, threshold=t, dilate_scaffold=r)
        fun = lp.calculate_scaffold(dgrids, mod.get_decoder_params(), size, gain=2.0, threshold=t, dilate_scaffold=r)
        assert torch.equal(got, fun) and got.dtype == torch.float32
        assert torch.equal(got.cpu(), oracle_occupancy(op, t, r))
        config.fused_module_ops = False
        try:
            old = mod.calculate_scaffold(dgrids, size, dev, threshold=t, dilate_scaffold=r)
        finally:
            config.fused_module_ops = True
        assert torch.equal(old, got), f"dilate {r}: the Renderer path and the fused path disagree"
    # the flat form goes the same way
    flat = torch.cat([g.reshape(-1, 16) for g in dgrids])
    sizes = [list(g.shape) for g in grids]
    assert torch.equal(mod.calculate_scaffold(flat, size, dev, threshold=t, grid_sizes=sizes, dilate_scaffold=1),
                       lp.calculate_scaffold(dgrids, mod.get_decoder_params(), size, gain=2.0, threshold=t, dilate_scaffold=1))


def test_memory_is_the_result_plus_one_byte_per_point():
    """Derived, not measured: the 4-byte result and the 1-byte workspace per lattice point, plus allocator rounding.  (The Renderer path
    holds origins, directions, near, far, a zero encoding, an int64 grid index and three outputs per point: about 50 MB here.)"""
    dev = _dev()
    mod = _module(dev)
    gen = torch.Generator().manual_seed(8)
    dgrids = [torch.randn(s, generator=gen).to(dev) for s in grid_sizes_for((1, 32, 32, 32, 16), True)]
    mod.calculate_scaffold(dgrids, [1, 2, 2, 2], dev)  # (library, kernels and the cached layer widths are loaded)
    n = 64 ** 3
    assert lp.scaffold_workspace_bytes([1, 64, 64, 64], 2) == n
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    sc = mod.calculate_scaffold(dgrids, [1, 64, 64, 64], dev, threshold=0.5)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated(dev) - before
    print(f"peak extra memory {extra} bytes for a result of {4 * n}")
    assert sc.shape == (1, 64, 64, 64)
    assert extra <= 1.25 * 4 * n + 64 * 1024, f"{extra} bytes beyond the inputs for a {4 * n}-byte scaffold"


def test_graph_capture_and_replay():
    """one calculate_scaffold with preallocated result and workspace, captured as a single linear chain (lattice kernel + three dilation
    passes); replayed on new grid values.  The threshold sits in a gap of the old AND the new values' upper opacities, so both
    scaffolds are sparse, different, and exactly the oracle's."""
    dev, c = _dev(), _case("triplane_c16_22x32_r1")
    grid, _, dec = _on(dev, c)  # (layer widths on the CPU: nothing in the call synchronises)
    size, r = c["size"], 1
    gen = torch.Generator().manual_seed(99)
    new = [0.5 * torch.randn(g.shape, generator=gen) for g in c["grids"]]
    op_new = oracle_opacity(new, c["dec"], size, GAIN)
    t, gap = unambiguous_threshold(torch.cat([c["op"].flatten(), op_new.flatten()]), 0.9, 0.97)
    assert gap > GAP, f"gap {gap:.3e}: change the seed"
    want_old, want_new = oracle_occupancy(c["op"], t, r), oracle_occupancy(op_new, t, r)
    assert not torch.equal(want_old, want_new) and 0 < float(want_new.mean()) < 1
    out = torch.empty(size, device=dev)
    ws = torch.empty(lp.scaffold_workspace_bytes(size, r), dtype=torch.uint8, device=dev)
    kw = dict(gain=GAIN, threshold=t, dilate_scaffold=r)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lp.calculate_scaffold(grid, dec, size, out=out, workspace=ws, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = lp.calculate_scaffold(grid, dec, size, out=out, workspace=ws, **kw)
    assert res is out
    out.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want_old)
    for g, v in zip(grid, new):  # new values in the tensors the graph reads
        g.copy_(v)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, lp.calculate_scaffold(grid, dec, size, **kw))
    assert torch.equal(out.cpu(), want_new)


def test_grid_beyond_4gb():
    """64-bit row arithmetic: the last batch element of a voxel grid-list begins 4 GB into its tensor.  Batch elements are independent
    scenes, so its opacity lattice has to equal, bit for bit, that of the same scene alone (which the tests above hold to the oracle);
    an offset that wrapped at 2^32 would read the zeros of an earlier element."""
    dev = _dev()
    shape = (128, 128, 128, 16)
    per = 4 * shape[0] * shape[1] * shape[2] * shape[3]
    batch = ((1 << 32) + per - 1) // per + 1
    gen = torch.Generator().manual_seed(21)
    small = torch.randn(1, *shape, generator=gen).to(dev)
    big = torch.zeros(batch, *shape, device=dev)
    big[batch - 1].copy_(small[0])
    assert (batch - 1) * per >= 1 << 32
    dec = _decoder(gen, 2, 2, 16, 32)
    ddec = lp.DecoderParams(dec.mlp_params.to(dev), dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
    got = lp.scaffold_opacity([big], ddec, [batch, 5, 6, 7], gain=GAIN)
    alone = lp.scaffold_opacity([small], ddec, [1, 5, 6, 7], gain=GAIN)
    assert torch.equal(got[batch - 1], alone[0])
    assert float((got[batch - 1] - got[0]).abs().max()) > 0  # (an empty element decodes to the bias alone)
    assert torch.equal(got[0], got[batch - 2])
    sc = lp.calculate_scaffold([big], ddec, [batch, 5, 6, 7], gain=GAIN, threshold=float(alone.median()), dilate_scaffold=1)
    assert torch.equal(sc[batch - 1], lp.calculate_scaffold([small], ddec, [1, 5, 6, 7], gain=GAIN, threshold=float(alone.median()),
                                                            dilate_scaffold=1)[0])


def test_fit_synthetic_scene_with_scaffold_steps():
    """the example with a scaffold schedule: the scaffold is rebuilt at the listed steps and every later render takes it"""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("fit_synthetic_scene", os.path.join(repo, "examples", "fit_synthetic_scene.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    old = lp.config.stop_transmittance
    try:
        r = mod.fit(steps=30, n_rays=2048, res=16, scaffold_steps=(10, 20), scaffold_size=24, scaffold_threshold=0.05)
        plain = mod.fit(steps=12, n_rays=2048, res=16)
    finally:
        lp.config.stop_transmittance = old
    print("fit with a scaffold:", r)
    assert r["scaffold_steps"] == [10, 20] and r["scaffold_shape"] == [1, 24, 24, 24]
    assert len(r["scaffold_occupancy"]) == 2 and all(0.0 < v <= 1.0 for v in r["scaffold_occupancy"])
    assert math.isfinite(r["heldout_psnr_db"]) and math.isfinite(r["last_loss"])
    assert "scaffold_steps" not in plain and math.isfinite(plain["last_loss"])  # (no flag: no scaffold anywhere)

"""CPU tests of the occupancy scaffold's host side: the lp_scaffold_* symbols and the ABI struct, every argument check of the C ABI
(each returns its code and message before anything touches a device), the workspace accounting, the Python wrappers' input checks,
and the identity the dilation rests on: max_pool3d followed by a threshold is a binary OR-dilation of the thresholded lattice."""
import ctypes

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib, grids, params, scaffold

FAKE = 0x10000  # a 16-byte-aligned non-NULL "device pointer": no check dereferences it, and every call below fails a check
OUT = 0x40000000  # fake result and workspace buffers far from it and from each other
WS = 0x80000000

DIMS_T, DIMS_O, DIMS_C = [16, 32, 32], [32, 32, 1], [32, 32, 16]


def _args(shape=(2, 6, 5, 7), dilate=1, sizes=((2, 1, 5, 7), (2, 6, 1, 7), (2, 6, 5, 1)), channels=16, dims_t=DIMS_T, dims_o=DIMS_O):
    descs, row = [], 0
    for s in sizes:
        descs.append(grids.GridDesc(*s, row))
        row += descs[-1].n_rows
    a = _lib.LpScaffoldArgs()
    a.grid = _lib.make_grid_list(None, descs, channels, row)
    a.grid.data = FAKE
    a.mlp_params = FAKE + 0x1000000
    a.n_mlp_params = sum(params.mlp_numel(d) for d in (dims_t, dims_o, DIMS_C))
    a.trunk, a.opacity = _lib.make_mlp(dims_t, 0), _lib.make_mlp(dims_o, params.mlp_numel(dims_t))
    a.gain, a.mask_out_of_bounds = 1.0, 0
    a.shape = _lib.LpGrid(*shape, 0, None)
    a.threshold, a.dilate = 0.5, dilate
    return a


def _err():
    return _lib.lib().lp_last_error().decode()


def _opacity(a, out=OUT):
    return _lib.lib().lp_scaffold_opacity(ctypes.byref(a), out, None)


def _build(a, out=OUT, ws=WS, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = a.shape.B * a.shape.D * a.shape.H * a.shape.W
    return _lib.lib().lp_scaffold_build(ctypes.byref(a), out, ws, ws_bytes, None)


CALLS = (_opacity, _build)


def test_symbols_struct_and_build_info():
    L = _lib.lib()
    for name in ("lp_scaffold_workspace_bytes", "lp_scaffold_opacity", "lp_scaffold_build"):
        assert hasattr(L, name), f"{name} not exported by liblightplane_hip.so"
    assert "lp_scaffold_opacity" in _lib.EXPORTS and "lp_scaffold_build" in _lib.EXPORTS
    assert L.lp_abi_sizeof(8) == ctypes.sizeof(_lib.LpScaffoldArgs)
    assert L.lp_abi_sizeof(9) == -1
    info = _lib.build_info()
    assert "scaffold" in info and "no atomics" in info["scaffold"]["dilation"] and "scalar loads" in info["scaffold"]["lattice"]
    assert "grid_resample" in info and "grid_tv" in info  # (its neighbours are still there)
    for name in ("calculate_scaffold", "scaffold_opacity", "scaffold_workspace_bytes"):
        assert name in lp.__all__ and getattr(lp, name) is getattr(scaffold, name)


def test_null_arguments_are_refused():
    L = _lib.lib()
    assert L.lp_scaffold_opacity(None, OUT, None) == -3 and "args is NULL" in _err()
    assert L.lp_scaffold_build(None, OUT, WS, 1 << 20, None) == -3 and "args is NULL" in _err()
    assert L.lp_scaffold_workspace_bytes(None) == -3 and "args is NULL" in _err()
    for call in CALLS:
        assert call(_args(), out=None) == -3 and "result pointer is NULL" in _err(), call.__name__
        a = _args()
        a.mlp_params = None
        assert call(a) == -3 and "mlp_params is NULL" in _err()
        a = _args()
        a.grid.data = None  # neither a flat tensor nor per-grid pointers
        assert call(a) == -3 and "grid.data is NULL" in _err()


def test_bad_scaffold_shapes_are_refused():
    L = _lib.lib()
    for field in ("B", "D", "H", "W"):
        for bad in (0, -3):
            a = _args()
            setattr(a.shape, field, bad)
            for call in CALLS:
                assert call(a) == -1 and "extent < 1" in _err(), (call.__name__, field, bad)
            assert L.lp_scaffold_workspace_bytes(ctypes.byref(a)) == -1 and "extent < 1" in _err()
    # the scaffold's batch is the grid-list's
    for call in CALLS:
        assert call(_args(shape=(3, 6, 5, 7))) == -1 and "scaffold batch 3 != grid batch 2" in _err(), call.__name__
    for bad in (-1, -7):
        a = _args(dilate=bad)
        for call in CALLS:
            assert call(a) == -1 and f"dilate = {bad}" in _err(), call.__name__
        assert L.lp_scaffold_workspace_bytes(ctypes.byref(a)) == -1 and f"dilate = {bad}" in _err()
    a = _args()
    a.threshold = float("nan")
    assert _build(a) == -1 and "threshold is NaN" in _err()


def test_grid_list_limits_are_the_samplers():
    for call in CALLS:
        assert call(_args(sizes=((2, 1, 1, 7),))) == -1 and "non-singular" in _err(), call.__name__  # a line is no sampler grid
        assert call(_args(sizes=((2, 6, 5, 7), (3, 1, 5, 7)))) == -1 and "batch 3 != 2" in _err()
        a = _args()
        a.grid.n_grids = 0
        assert call(a) == -1 and "empty grid-list" in _err()
        assert call(_args(channels=129, dims_t=[129, 32, 32])) == -2 and "channels" in _err()


def test_decoders_that_do_not_chain_are_refused():
    for call in CALLS:
        assert call(_args(dims_t=[32, 32, 32])) == -1 and "trunk MLP input width 32 != grid channels 16" in _err(), call.__name__
        assert call(_args(dims_o=[16, 32, 1])) == -1 and "opacity MLP input width 16 != 32" in _err()
        assert call(_args(dims_o=[32, 32, 2])) == -1 and "must end in 1 output" in _err()
        assert call(_args(dims_t=[], dims_o=[32, 32, 1])) == -1 and "opacity MLP input width 32 != 16" in _err()  # two-grid mode: C
        assert call(_args(dims_o=[])) == -1 and "opacity MLP has no layers" in _err()
        assert call(_args(dims_t=[16, 200, 32])) == -2 and "width 200" in _err()
        a = _args()
        a.opacity.offset += 1
        assert call(a) == -1 and "flat layout" in _err()
        a = _args()
        a.n_mlp_params = params.mlp_numel(DIMS_T) + params.mlp_numel(DIMS_O) - 1
        assert call(a) == -1 and "mlp_params has" in _err()
        # the colour MLP behind the two is never read: a vector that ends with the opacity head passes on to the next check
        a = _args()
        a.n_mlp_params = params.mlp_numel(DIMS_T) + params.mlp_numel(DIMS_O)
        assert call(a, out=None) == -3 and "result pointer" in _err()


def test_under_aligned_pointers_are_refused():
    for call in CALLS:
        for off in (4, 8, 2):
            a = _args()
            a.grid.data = FAKE + off
            assert call(a) == -1 and "grid.data" in _err() and "16-byte aligned" in _err(), (call.__name__, off)
            a = _args()
            a.grid.grids[1].data = FAKE + 0x100000 + off
            assert call(a) == -1 and "grid.grids[1].data" in _err() and "16-byte aligned" in _err()
            a = _args()
            a.mlp_params = FAKE + 0x1000000 + off
            assert call(a) == -1 and "mlp_params" in _err() and "16-byte aligned" in _err()
            assert call(_args(), out=OUT + off) == -1 and "16-byte aligned" in _err()
    assert _build(_args(), ws=WS + 4) == -1 and "workspace" in _err() and "16-byte aligned" in _err()


def test_workspace_is_checked_when_bytes_are_needed():
    a = _args(dilate=2)
    n = 2 * 6 * 5 * 7
    assert _build(a, ws=None) == -1 and "workspace is NULL" in _err() and str(n) in _err()
    assert _build(a, ws_bytes=n - 1) == -1 and f"workspace of {n - 1} bytes" in _err()
    assert _build(a, ws=OUT + 16) == -1 and "overlaps the result" in _err()
    assert _build(a, ws=OUT + 4 * n - 16) == -1 and "overlaps the result" in _err()
    # without a dilation no workspace is needed: a NULL one passes on to the next check (here: the result pointer)
    assert _build(_args(dilate=0), out=None, ws=None, ws_bytes=0) == -3 and "result pointer" in _err()


def test_workspace_bytes_is_at_most_one_byte_per_point():
    L = _lib.lib()
    for shape in ((2, 6, 5, 7), (1, 3, 2, 70), (1, 1, 1, 1), (2, 9, 1, 5), (1, 256, 256, 256), (3, 1024, 1024, 1024)):
        n = shape[0] * shape[1] * shape[2] * shape[3]
        for r in (0, 1, 2, 3, 100, 5000):
            got = lp.scaffold_workspace_bytes(shape, r)
            assert 0 <= got <= n, (shape, r, got)
            assert got == (n if r > 0 else 0)
            a = _args(shape=(2,) + tuple(shape[1:]), dilate=r)
            assert L.lp_scaffold_workspace_bytes(ctypes.byref(a)) == (2 * n // shape[0] if r > 0 else 0)
    assert lp.scaffold_workspace_bytes(torch.tensor([2, 3, 4, 5]), 1) == 120
    with pytest.raises(AssertionError, match="positive \\[B, D, H, W\\]"):
        lp.scaffold_workspace_bytes([2, 0, 4, 5], 1)
    with pytest.raises(AssertionError, match="dilate"):
        lp.scaffold_workspace_bytes([2, 3, 4, 5], -1)


def _or_dilate(occ, r):
    """separable binary dilation, the way the kernels do it: per axis, OR over the window [i - r, i + r] clipped to the axis"""
    out = occ.clone()
    for ax in (3, 2, 1):
        n = out.shape[ax]
        src = out.clone()
        for i in range(n):
            lo, hi = max(i - r, 0), min(i + r, n - 1)
            out.select(ax, i).copy_(src.narrow(ax, lo, hi - lo + 1).any(dim=ax))
    return out


@pytest.mark.parametrize("shape", [(2, 6, 5, 7), (1, 3, 2, 70), (1, 1, 1, 1), (2, 9, 1, 5)])
@pytest.mark.parametrize("r", [0, 1, 2, 3, 9, 80])
def test_threshold_commutes_with_the_max_pool(shape, r):
    """max_pool3d(v, 2 r + 1, stride 1, padding r) > t  ==  OR-dilation of (v > t): the pool pads with -inf, which never wins, and
    max commutes with the monotone map v -> v > t.  r >= the axis size: the window covers the whole axis.  (max_pool3d itself asks
    for padding <= kernel / 2, which 2 r + 1 always satisfies.)"""
    gen = torch.Generator().manual_seed(11 + r)
    v = torch.rand(shape, generator=gen) ** 3  # most values small: a sparse occupancy
    for t in (0.05, 0.4, 0.9, -1.0, 2.0):  # (-1: everything occupied, 2: nothing)
        want = v > t
        if r > 0:
            want = torch.nn.functional.max_pool3d(v, kernel_size=2 * r + 1, padding=r, stride=1) > t
        got = _or_dilate(v > t, r)
        assert torch.equal(got, want), (shape, r, t)


def test_wrappers_reject_bad_arguments():
    dec = lp.init_decoder_params(device="cpu", n_layers_opacity=2, n_layers_trunk=2, n_layers_color=2, input_chn=8, hidden_chn=16,
                                 color_chn=3)
    g = torch.zeros(2, 3, 4, 5, 8)
    for fn in (lp.calculate_scaffold, lp.scaffold_opacity):
        for bad in ((g,), "grid", None):
            with pytest.raises(NotImplementedError):
                fn(bad, dec, [2, 4, 4, 4])
        with pytest.raises(AssertionError, match="grid_sizes cannot be None"):
            fn(g.reshape(-1, 8), dec, [2, 4, 4, 4])
        with pytest.raises(AssertionError, match="positive \\[B, D, H, W\\]"):
            fn([g], dec, [2, 4, 0, 4])
        with pytest.raises(AssertionError, match="positive \\[B, D, H, W\\]"):
            fn([g], dec, [4, 4, 4])
        with pytest.raises(AssertionError, match="float32"):
            fn([g.double()], dec, [2, 4, 4, 4])
        with pytest.raises(AssertionError, match="contiguous"):
            fn([torch.zeros(2, 3, 4, 8, 5).transpose(3, 4)], dec, [2, 4, 4, 4])
        # there is no CPU path: tensors that pass every check still need a GPU
        with pytest.raises(_lib.LightplaneHipError, match="GPU only"):
            fn([g], dec, [2, 4, 4, 4])
    with pytest.raises(AssertionError, match="dilate_scaffold has to be >= 0"):
        lp.calculate_scaffold([g], dec, [2, 4, 4, 4], dilate_scaffold=-1)


def test_module_keeps_its_signature_and_its_cpu_behaviour():
    """LightplaneRenderer.calculate_scaffold: same parameters and defaults as before; a grid that is not on a GPU never reaches the fused
    function (the present path then raises what it always raised: there is no CPU path)."""
    import inspect
    from lightplane_amd.modules import _fused_scaffold_supported
    sig = inspect.signature(lp.LightplaneRenderer.calculate_scaffold)
    assert list(sig.parameters) == ["self", "feature_grid", "scaffold_size", "device", "threshold", "grid_sizes", "dilate_scaffold"]
    assert sig.parameters["threshold"].default == 1e-7 and sig.parameters["dilate_scaffold"].default == 2
    assert sig.parameters["grid_sizes"].default is None
    g = torch.zeros(1, 1, 4, 4, 16)
    assert not _fused_scaffold_supported([g], "cpu") and not _fused_scaffold_supported([g], "cuda:0")
    assert not _fused_scaffold_supported(g.reshape(-1, 16), torch.device("cpu"))
    assert not _fused_scaffold_supported([], "cuda:0") and not _fused_scaffold_supported([None], "cuda:0")

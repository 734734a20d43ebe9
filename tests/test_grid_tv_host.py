"""CPU tests of the total-variation regulariser's host side: the lp_grid_tv_* symbols, every argument check of the C ABI (each returns
its code and message before anything touches a device), the workspace query, and the Python wrappers' input checks."""
import ctypes

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib, grids, regularizers

FAKE = 0x10000  # a 16-byte-aligned non-NULL "device pointer": no check dereferences it, and every call below fails a check


def _list(sizes=((2, 9, 7, 5),), channels=16, flat=True):
    descs, row = [], 0
    for s in sizes:
        descs.append(grids.GridDesc(*s, row))
        row += descs[-1].n_rows
    gl = _lib.make_grid_list(None, descs, channels, row)
    if flat:
        gl.data = FAKE
    else:
        for g in range(len(descs)):
            gl.grids[g].data = FAKE + 0x1000000 * (g + 1)
            gl.grids[g].row_offset = 0
    return gl


def _err():
    return _lib.lib().lp_last_error().decode()


def test_symbols_exist_and_build_info_names_the_capability():
    L = _lib.lib()
    for name in ("lp_grid_tv_workspace_bytes", "lp_grid_tv_forward", "lp_grid_tv_backward", "lp_grid_tv_fused"):
        assert hasattr(L, name), f"{name} not exported by liblightplane_hip.so"
    info = _lib.build_info()
    assert "grid_tv" in info and info["grid_tv"]["p"] == [1, 2]
    for name in ("grid_tv_loss", "add_grid_tv_grad_", "grid_tv_workspace_bytes"):
        assert name in lp.__all__ and getattr(lp, name) is getattr(regularizers, name)


def test_workspace_bytes_positive_and_monotone_in_the_row_count():
    L = _lib.lib()
    last = 0
    for n in (1, 2, 3, 5, 8, 13, 16, 17, 31, 32, 33, 64, 100, 128, 256, 512):
        for C in (1, 3, 16, 32, 128):
            gl = _list(((1, n, n, n),), C)
            b = L.lp_grid_tv_workspace_bytes(ctypes.byref(gl))
            assert b > 0 and b % 8 == 0
        gl = _list(((1, n, n, n),), 32)
        b = L.lp_grid_tv_workspace_bytes(ctypes.byref(gl))
        assert b >= last, (n, b, last)
        last = b
    # growing any single extent never shrinks it, and a list needs the sum of its entries
    base = (2, 20, 30, 40)
    b0 = lp.grid_tv_workspace_bytes([list(base) + [32]])
    for ax in range(4):
        for inc in (1, 7, 100):
            s = list(base)
            s[ax] += inc
            assert lp.grid_tv_workspace_bytes([s + [32]]) >= b0
    planes = [[2, 1, 30, 40, 32], [2, 20, 1, 40, 32], [2, 20, 30, 1, 32]]
    assert lp.grid_tv_workspace_bytes(planes) == sum(lp.grid_tv_workspace_bytes([s]) for s in planes)
    # the cfg-5 grid: a small fraction of the 2.15 GB it regularises
    assert lp.grid_tv_workspace_bytes([[1, 256, 256, 256, 32]]) <= 2 << 20


def test_workspace_query_rejects_malformed_lists():
    L = _lib.lib()
    assert L.lp_grid_tv_workspace_bytes(None) == -3 and "NULL" in _err()
    gl = _list()
    gl.n_grids = 0
    assert L.lp_grid_tv_workspace_bytes(ctypes.byref(gl)) == -1 and "n_grids" in _err()
    gl = _list()
    gl.grids[0].H = 0
    assert L.lp_grid_tv_workspace_bytes(ctypes.byref(gl)) == -1 and "non-positive extent" in _err()
    gl = _list(channels=129)
    assert L.lp_grid_tv_workspace_bytes(ctypes.byref(gl)) == -2 and "channels" in _err()
    gl = _list(((1, 2048, 1024, 1024),))  # 2^31 rows
    assert L.lp_grid_tv_workspace_bytes(ctypes.byref(gl)) == -2 and "2^31" in _err()
    with pytest.raises(_lib.LightplaneHipError, match="2\\^31"):
        lp.grid_tv_workspace_bytes([[1, 2048, 1024, 1024, 16]])
    # lines and single cells are grids here (the samplers refuse them)
    assert L.lp_grid_tv_workspace_bytes(ctypes.byref(_list(((3, 1, 1, 11), (1, 1, 1, 1))))) > 0


def _fwd(gl, w=None, nw=0, p=1, loss=FAKE, ws=FAKE, ws_bytes=None):
    L = _lib.lib()
    if ws_bytes is None:
        ws_bytes = L.lp_grid_tv_workspace_bytes(ctypes.byref(gl))
    return L.lp_grid_tv_forward(ctypes.byref(gl), w, nw, p, loss, ws, ws_bytes, None)


def _bwd(gl, w=None, nw=0, p=1, grad=FAKE + 0x100, grad_list=None, n=0, accumulate=0):
    return _lib.lib().lp_grid_tv_backward(ctypes.byref(gl), w, nw, p, None, 1.0, grad, grad_list, n, accumulate, None)


def _fused(gl, w=None, nw=0, p=1, loss=FAKE, ws=FAKE, ws_bytes=None, grad=FAKE + 0x100, grad_list=None, n=0):
    L = _lib.lib()
    if ws_bytes is None:
        ws_bytes = L.lp_grid_tv_workspace_bytes(ctypes.byref(gl))
    return L.lp_grid_tv_fused(ctypes.byref(gl), w, nw, p, loss, ws, ws_bytes, None, 1.0, grad, grad_list, n, None)


def test_p_outside_1_2_is_refused():
    gl = _list()
    for call in (_fwd, _bwd, _fused):
        for p in (0, 3, -1):
            assert call(gl, p=p) == -1 and "p = " in _err(), call.__name__


def test_null_pointers_are_refused():
    L = _lib.lib()
    gl = _list()
    assert L.lp_grid_tv_forward(None, None, 0, 1, FAKE, FAKE, 1 << 20, None) == -3 and "grid-list is NULL" in _err()
    assert L.lp_grid_tv_backward(None, None, 0, 1, None, 1.0, FAKE, None, 0, 0, None) == -3
    assert L.lp_grid_tv_fused(None, None, 0, 1, FAKE, FAKE, 1 << 20, None, 1.0, FAKE, None, 0, None) == -3
    for call in (_fwd, _fused):
        assert call(gl, loss=None) == -3 and "loss is NULL" in _err()
        assert call(gl, ws=None) == -3 and "workspace is NULL" in _err()
    for call in (_bwd, _fused):
        assert call(gl, grad=None) == -3 and "gradient" in _err()
    nodata = _list()
    nodata.data = None  # neither a flat tensor nor per-grid pointers
    for call in (_fwd, _bwd, _fused):
        assert call(nodata) == -3 and "data pointer" in _err()


def test_short_or_misaligned_workspace_is_refused():
    gl = _list()
    need = _lib.lib().lp_grid_tv_workspace_bytes(ctypes.byref(gl))
    for call in (_fwd, _fused):
        assert call(gl, ws_bytes=need - 1) == -1 and "workspace of" in _err() and str(need) in _err()
        assert call(gl, ws_bytes=0) == -1
        assert call(gl, ws=FAKE + 4) == -1 and "aligned" in _err()


def test_weight_count_has_to_match_the_list():
    gl = _list(((2, 1, 7, 5), (2, 9, 1, 5), (2, 9, 7, 1)))
    w2 = (ctypes.c_float * 2)(1.0, 2.0)
    w3 = (ctypes.c_float * 3)(1.0, 2.0, 3.0)
    for call in (_fwd, _bwd, _fused):
        assert call(gl, w=w2, nw=2) == -1 and "grid weights" in _err()
        assert call(gl, w=w3, nw=4) == -1
        assert call(gl, w=None, nw=3) == -1
        assert call(gl, w=w3, nw=3, p=7) == -1 and "p = " in _err()  # a matching count passes on to the next check


def test_gradient_list_has_to_match_the_grid_list():
    # per-grid base pointers: every grid needs its own gradient entry
    gl = _list(((2, 1, 7, 5), (2, 9, 1, 5), (2, 9, 7, 1)), flat=False)
    two = (ctypes.c_void_p * 2)(FAKE + 0x100, FAKE + 0x200)
    three = (ctypes.c_void_p * 3)(FAKE + 0x100, FAKE + 0x200, FAKE + 0x300)
    hole = (ctypes.c_void_p * 3)(FAKE + 0x100, None, FAKE + 0x300)
    for call in (_bwd, _fused):
        assert call(gl, grad=None, grad_list=two, n=2) == -1 and "gradient list of 2 entries for 3 grids" in _err()
        assert call(gl, grad=None, grad_list=three, n=2) == -1
        assert call(gl, grad=None, grad_list=None, n=3) == -1
        assert call(gl, grad=None, grad_list=hole, n=3) == -1 and "no gradient buffer for grid 1" in _err()
        assert call(gl, grad=FAKE + 0x100, grad_list=None, n=0) == -1 and "own gradient entry" in _err()  # a flat buffer cannot serve them
        assert call(gl, grad=None, grad_list=three, n=3, p=5) == -1 and "p = " in _err()  # a matching list passes on
    # a gradient that is the grid itself
    flat = _list()
    for call in (_bwd, _fused):
        assert call(flat, grad=FAKE) == -1 and "aliases" in _err()


def test_wrappers_reject_what_the_renderer_rejects():
    g = torch.zeros(2, 3, 4, 5, 8)
    for bad in ((g,), "grid", None):
        with pytest.raises(NotImplementedError):
            lp.grid_tv_loss(bad)
        with pytest.raises(NotImplementedError):
            lp.add_grid_tv_grad_(bad, [torch.zeros_like(g)])
    flat = g.reshape(-1, 8)
    with pytest.raises(AssertionError, match="grid_sizes cannot be None"):
        lp.grid_tv_loss(flat)
    with pytest.raises(AssertionError, match="grid_sizes cannot be None"):
        lp.add_grid_tv_grad_(flat, torch.zeros_like(flat))
    with pytest.raises(AssertionError, match="compatible"):
        lp.grid_tv_loss(flat, grid_sizes=[[2, 3, 4, 5, 4]])
    with pytest.raises(AssertionError, match="p has to be"):
        lp.grid_tv_loss([g], p=3)
    with pytest.raises(AssertionError, match="grid_weights"):
        lp.grid_tv_loss([g], grid_weights=[1.0, 2.0])
    with pytest.raises(AssertionError, match="one tensor per grid"):
        lp.add_grid_tv_grad_([g], torch.zeros_like(g))
    with pytest.raises(AssertionError, match="shaped like its grid"):
        lp.add_grid_tv_grad_([g], [torch.zeros(2, 3, 4, 5, 4)])
    with pytest.raises(AssertionError, match="float32"):
        lp.grid_tv_loss([g.double()])
    # there is no CPU path: tensors that pass every check still need a GPU
    with pytest.raises(_lib.LightplaneHipError, match="GPU only"):
        lp.grid_tv_loss([g])

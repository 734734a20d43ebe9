"""CPU tests of the grid-list resampling's host side: the lp_grid_resample_* symbols, every argument check of the C ABI (each returns
its code and message before anything touches a device), the Python wrappers' input checks and the output-size rule."""
import ctypes
import math

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib, grids, resample

FAKE = 0x10000  # a 16-byte-aligned non-NULL "device pointer": no check dereferences it, and every call below fails a check
FAR = 0x40000000  # a second fake buffer far from the first


def _list(sizes=((2, 9, 7, 5),), channels=16, flat=True, base=FAKE):
    descs, row = [], 0
    for s in sizes:
        descs.append(grids.GridDesc(*s, row))
        row += descs[-1].n_rows
    gl = _lib.make_grid_list(None, descs, channels, row)
    if flat:
        gl.data = base
    else:
        for g in range(len(descs)):
            gl.grids[g].data = base + 0x1000000 * (g + 1)
            gl.grids[g].row_offset = 0
    return gl


def _err():
    return _lib.lib().lp_last_error().decode()


def _fwd(src, dst, align=0, coeffs=None):
    return _lib.lib().lp_grid_resample_forward(ctypes.byref(src), ctypes.byref(dst), align, coeffs, None)


def _bwd(src, dst, align=0, coeffs=None, accumulate=0):
    return _lib.lib().lp_grid_resample_backward(ctypes.byref(src), ctypes.byref(dst), align, coeffs, accumulate, None)


CALLS = (_fwd, _bwd)
SRC = ((2, 9, 7, 5),)
DST = ((2, 18, 14, 10),)


def test_symbols_exist_and_build_info_names_the_capability():
    L = _lib.lib()
    for name in ("lp_grid_resample_forward", "lp_grid_resample_backward"):
        assert hasattr(L, name), f"{name} not exported by liblightplane_hip.so"
        assert name in _lib.EXPORTS
    assert L.lp_version() == 207  # additive: no version change
    info = _lib.build_info()
    assert "grid_resample" in info and "no atomics" in info["grid_resample"]["adjoint"]
    assert "grid_tv" in info  # (its neighbour is still there)
    for name in ("grid_resample", "grid_up_sample"):
        assert name in lp.__all__ and getattr(lp, name) is getattr(resample, name)


def test_null_structs_are_refused():
    L = _lib.lib()
    gl = _list()
    assert L.lp_grid_resample_forward(None, ctypes.byref(gl), 0, None, None) == -3 and "source grid-list is NULL" in _err()
    assert L.lp_grid_resample_forward(ctypes.byref(gl), None, 0, None, None) == -3 and "destination grid-list is NULL" in _err()
    assert L.lp_grid_resample_backward(None, ctypes.byref(gl), 0, None, 0, None) == -3 and "NULL" in _err()
    assert L.lp_grid_resample_backward(ctypes.byref(gl), None, 0, None, 0, None) == -3 and "NULL" in _err()
    nodata = _list(SRC)
    nodata.data = None  # neither a flat tensor nor per-grid pointers
    for call in CALLS:
        assert call(nodata, _list(DST, base=FAR)) == -3 and "data pointer" in _err()
        assert call(_list(SRC), nodata) == -3 and "data pointer" in _err()


def test_lists_have_to_match_in_count_batch_and_channels():
    for call in CALLS:
        two = _list(((2, 9, 7, 5), (2, 1, 7, 5)))
        assert call(two, _list(DST, base=FAR)) == -1 and "2 source grids for 1 destination grids" in _err(), call.__name__
        assert call(_list(SRC, 16), _list(DST, 32, base=FAR)) == -1 and "16 source channels for 32 destination channels" in _err()
        assert call(_list(SRC), _list(((3, 18, 14, 10),), base=FAR)) == -1 and "batch size 2 of the source, 3 of the destination" in _err()
        zero = _list(SRC)
        zero.n_grids = 0
        assert call(zero, _list(DST, base=FAR)) == -1 and "n_grids" in _err()
        assert call(_list(SRC, 129), _list(DST, 129, base=FAR)) == -2 and "channels" in _err()


def test_empty_extents_are_refused():
    for call in CALLS:
        for field in ("B", "D", "H", "W"):
            for which in (0, 1):
                src, dst = _list(SRC), _list(DST, base=FAR)
                setattr((src, dst)[which].grids[0], field, 0)
                assert call(src, dst) == -1 and "empty extent" in _err(), (call.__name__, field, which)
    # lines and single cells are grids here (the samplers refuse them): such a call passes on to the next check
    assert _fwd(_list(((3, 1, 1, 11),)), _list(((3, 1, 1, 22),), base=FAR), align=2) == -1 and "align_corners" in _err()


def test_align_corners_outside_0_1_is_refused():
    for call in CALLS:
        for bad in (2, -1, 7):
            assert call(_list(SRC), _list(DST, base=FAR), align=bad) == -1 and f"align_corners = {bad}" in _err(), call.__name__


def test_coefficients_have_to_be_finite_and_positive():
    for call in CALLS:
        for pos, bad in ((0, 0.0), (1, -0.5), (2, float("inf")), (1, float("nan")), (0, float("-inf"))):
            c = [0.5, 0.5, 0.5]
            c[pos] = bad
            co = (ctypes.c_float * 3)(*c)
            assert call(_list(SRC), _list(DST, base=FAR), coeffs=co) == -1, (call.__name__, bad)
            assert "coordinate coefficient %d" % pos in _err() and "finite and positive" in _err() and "axis %s" % "DHW"[pos] in _err()
        # the second grid's coefficients are looked at too
        two_s = _list(((2, 9, 7, 5), (2, 1, 7, 5)), flat=False)
        two_d = _list(((2, 18, 14, 10), (2, 1, 14, 10)), flat=False, base=FAR)
        co = (ctypes.c_float * 6)(0.5, 0.5, 0.5, 0.5, -1.0, 0.5)
        assert call(two_s, two_d, coeffs=co) == -1 and "coordinate coefficient 4 (grid 1, axis H)" in _err()


def test_tensors_of_2_to_the_31_rows_are_refused():
    big = ((1, 2048, 1024, 1024),)  # 2^31 rows
    for call in CALLS:
        assert call(_list(((1, 1024, 512, 512),)), _list(big, base=FAR)) == -1 and "destination" in _err() and "2^31" in _err()
        assert call(_list(big), _list(((1, 1024, 512, 512),), base=FAR)) == -1 and "source" in _err() and "2^31" in _err()


def test_a_source_that_aliases_its_destination_is_refused():
    for call in CALLS:
        assert call(_list(SRC), _list(DST)) == -1 and "aliases" in _err(), call.__name__
        # overlap anywhere counts: the destination begins inside the source
        assert call(_list(SRC), _list(DST, base=FAKE + 64)) == -1 and "source grid 0 aliases destination grid 0" in _err()
        # ... and between different positions of per-grid lists
        src = _list(((2, 9, 7, 5), (2, 1, 7, 5)), flat=False)
        dst = _list(((2, 18, 14, 10), (2, 1, 14, 10)), flat=False, base=FAR)
        dst.grids[0].data = src.grids[1].data
        assert call(src, dst) == -1 and "source grid 1 aliases destination grid 0" in _err()
        # buffers that only touch do not alias: the call passes on to the next check
        end = FAKE + 2 * 9 * 7 * 5 * 16 * 4
        assert call(_list(SRC), _list(DST, base=end), align=3) == -1 and "align_corners" in _err()


def test_pointers_have_to_be_4_byte_aligned():
    for call in CALLS:
        for off in (1, 2, 3):
            assert call(_list(SRC, base=FAKE + off), _list(DST, base=FAR)) == -1 and "4-byte aligned" in _err(), (call.__name__, off)
            assert call(_list(SRC), _list(DST, base=FAR + off)) == -1 and "4-byte aligned" in _err()
        # 4-byte aligned is enough (the scalar path takes it): the call passes on to the next check
        assert call(_list(SRC, base=FAKE + 4), _list(DST, base=FAR + 8), align=5) == -1 and "align_corners" in _err()


def test_wrappers_reject_bad_arguments():
    g = torch.zeros(2, 3, 4, 5, 8)
    for bad in ((g,), "grid", None):
        with pytest.raises(NotImplementedError):
            lp.grid_resample(bad, scale_factor=2.0)
    with pytest.raises(AssertionError, match="takes a list"):
        lp.grid_up_sample((g,))
    with pytest.raises(AssertionError, match="exactly one of sizes and scale_factor"):
        lp.grid_resample([g])
    with pytest.raises(AssertionError, match="exactly one of sizes and scale_factor"):
        lp.grid_resample([g], sizes=[6, 8, 10], scale_factor=2.0)
    flat = g.reshape(-1, 8)
    with pytest.raises(AssertionError, match="grid_sizes cannot be None"):
        lp.grid_resample(flat, scale_factor=2.0)
    with pytest.raises(AssertionError, match="compatible"):
        lp.grid_resample(flat, [[2, 3, 4, 5, 4]], scale_factor=2.0)
    with pytest.raises(AssertionError, match="sizes has 2 entries for 1 grids"):
        lp.grid_resample([g], sizes=[[6, 8, 10], [6, 8, 10]])
    with pytest.raises(AssertionError, match="positive \\[D, H, W\\]"):
        lp.grid_resample([g], sizes=[[6, 0, 10]])
    with pytest.raises(AssertionError, match="scale_factor has to be positive"):
        lp.grid_resample([g], scale_factor=0.0)
    with pytest.raises(AssertionError, match="empty axis"):
        lp.grid_resample([g], scale_factor=0.3)
    with pytest.raises(AssertionError, match="float32"):
        lp.grid_resample([g.double()], scale_factor=2.0)
    with pytest.raises(AssertionError, match="contiguous"):
        lp.grid_resample([torch.zeros(2, 3, 4, 8, 5).transpose(3, 4)], scale_factor=2.0)
    # there is no CPU path: tensors that pass every check still need a GPU
    with pytest.raises(_lib.LightplaneHipError, match="GPU only"):
        lp.grid_resample([g], scale_factor=2.0)
    with pytest.raises(_lib.LightplaneHipError, match="GPU only"):
        lp.grid_resample(flat, [[2, 3, 4, 5, 8]], sizes=[6, 8, 10])
    grids_ = [g]
    with pytest.raises(_lib.LightplaneHipError, match="GPU only"):
        lp.grid_up_sample(grids_)
    assert grids_[0] is g  # a failed call leaves the list as it was


def test_output_size_rule():
    sizes = [[2, 9, 7, 5, 16], [2, 1, 7, 5, 16], [2, 9, 1, 5, 16], [2, 9, 7, 1, 16], [2, 1, 1, 5, 16]]
    assert lp.resampled_sizes(sizes, 2.0) == [[2, 18, 14, 10, 16], [2, 1, 14, 10, 16], [2, 18, 1, 10, 16], [2, 18, 14, 1, 16],
                                              [2, 1, 1, 10, 16]]
    # floor(n * factor); singular axes stay singular whatever the factor
    assert lp.resampled_sizes(sizes, 1.5) == [[2, 13, 10, 7, 16], [2, 1, 10, 7, 16], [2, 13, 1, 7, 16], [2, 13, 10, 1, 16],
                                              [2, 1, 1, 7, 16]]
    assert lp.resampled_sizes([[1, 300, 33, 2, 4]], 1.7) == [[1, 510, 56, 3, 4]]
    assert lp.resampled_sizes([[1, 9, 7, 5, 4]], 0.5) == [[1, 4, 3, 2, 4]]
    for n in range(2, 40):
        for f in (1.1, 1.5, 2.0, 2.5, 3.0):
            assert lp.resampled_sizes([[1, n, 1, n, 3]], f) == [[1, math.floor(n * f), 1, math.floor(n * f), 3]]
    # explicit sizes: one triple for every grid, or one per grid; batch and channels are kept
    assert resample._target_sizes(sizes[:2], [4, 5, 6], None) == [[2, 4, 5, 6, 16], [2, 4, 5, 6, 16]]
    assert resample._target_sizes(sizes[:2], [[4, 5, 6], [1, 2, 3]], None) == [[2, 4, 5, 6, 16], [2, 1, 2, 3, 16]]
    # only a scale factor without align_corners sets the coordinate coefficient itself: float(1 / factor) on every axis
    assert resample._coeffs(2, None, False) is None and resample._coeffs(2, 1.5, True) is None
    co = resample._coeffs(2, 1.5, False)
    assert len(co) == 6 and all(v == ctypes.c_float(1.0 / 1.5).value for v in co)

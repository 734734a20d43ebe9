"""CPU tests of the host side of the gather / splat at points: the lp_point_* symbols and the ABI struct, every argument check of the
four entry points (each returns its code and message before anything touches a device), the Python wrappers' input checks, and the
admissibility of the GPU tests' inputs (tests/point_grid_cases.py), computed from the oracle alone."""
import ctypes
import inspect

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib, grids, point_grid
from tests import point_grid_cases as PG

FAKE = 0x10000  # 16-byte-aligned non-NULL "device pointers" far from each other: no check dereferences them, and every call below
STEP = 0x1000000  # fails a check (or has no points to launch for)

TRIPLANE = ((2, 1, 5, 7), (2, 6, 1, 7), (2, 6, 5, 1))
ENTRIES = ("lp_point_gather", "lp_point_splat", "lp_point_normalize", "lp_point_grad_points")


def _args(sizes=TRIPLANE, channels=16, vec_channels=None, n_rays=3, n_pts=5, weights=True):
    a = _lib.LpPointGridArgs()
    descs, row = [], 0
    for s in sizes:
        descs.append(grids.GridDesc(*s, row))
        row += descs[-1].n_rows
    a.grid = _lib.make_grid_list(None, descs, channels, row)
    a.grid.data = FAKE
    if weights:
        for g in range(len(sizes)):
            a.row_weight[g] = FAKE + STEP
    a.points, a.grid_idx, a.vectors = FAKE + 2 * STEP, FAKE + 3 * STEP, FAKE + 4 * STEP
    a.out_features, a.grad_points = FAKE + 5 * STEP, FAKE + 6 * STEP
    a.n_rays, a.n_pts = n_rays, n_pts
    a.channels = channels if vec_channels is None else vec_channels
    return a


def _err():
    return _lib.lib().lp_last_error().decode()


def _call(name, a):
    return getattr(_lib.lib(), name)(ctypes.byref(a), None)


def test_symbols_struct_and_exports():
    L = _lib.lib()
    for name in ENTRIES:
        assert hasattr(L, name), f"{name} not exported by liblightplane_hip.so"
        assert name in _lib.EXPORTS
    assert L.lp_abi_sizeof(14) == ctypes.sizeof(_lib.LpPointGridArgs)
    for which in (9, 11, 13, 15, 99):
        assert L.lp_abi_sizeof(which) == -1, which
    assert L.lp_abi_sizeof(10) == ctypes.sizeof(_lib.LpPointsArgs) and L.lp_abi_sizeof(12) == ctypes.sizeof(_lib.LpRayClipArgs)
    assert L.lp_version() == 207  # additive: no version change
    info = _lib.build_info()
    assert set(info["point_grid"]) == {"gather", "splat", "normalize", "grad_points"}
    assert "points" in info and "ray_clip" in info and "scaffold" in info  # (its neighbours are still there)
    for name in ("sample_grid_at_points", "splat_points"):
        assert name in lp.__all__ and getattr(lp, name) is getattr(point_grid, name)


def test_signatures():
    sig = inspect.signature(lp.sample_grid_at_points)
    assert list(sig.parameters) == ["points", "grid", "ray_grid_idx", "mask_out_of_bounds_samples", "contract_coords", "grid_sizes"]
    assert sig.parameters["grid_sizes"].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(lp.splat_points)
    assert list(sig.parameters) == ["points", "features", "output_grid_size", "ray_grid_idx", "mask_out_of_bounds_samples",
                                    "contract_coords", "normalize", "return_list"]
    assert sig.parameters["normalize"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["normalize"].default is True
    assert sig.parameters["return_list"].default is True


def test_empty_batches_return_ok_without_a_launch():
    for name in ENTRIES:
        assert _call(name, _args(n_rays=0)) == 0, (name, _err())
        assert _call(name, _args(n_pts=0)) == 0, (name, _err())
        a = _args(n_rays=0)  # (an empty batch has no tensors to point at)
        a.points = a.grid_idx = a.vectors = a.out_features = a.grad_points = None
        assert _call(name, a) == 0, (name, _err())
        if name != "lp_point_normalize":  # (which needs its weights whatever the batch)
            assert _call(name, _args(n_rays=0, weights=False)) == 0, (name, _err())


def test_null_arguments_are_refused():
    L = _lib.lib()
    for name in ENTRIES:
        assert getattr(L, name)(None, None) == -3 and "args is NULL" in _err(), name
        a = _args()
        a.grid.data = None  # neither a flat tensor nor per-grid pointers
        assert _call(name, a) == -3 and "grid.data is NULL" in _err(), name
    required = {"lp_point_gather": ("points", "grid_idx", "out_features"), "lp_point_splat": ("points", "grid_idx", "vectors"),
                "lp_point_grad_points": ("points", "grid_idx", "vectors", "grad_points")}
    for name, fields in required.items():
        for field in fields:
            a = _args()
            setattr(a, field, None)
            msg = "points / grid_idx is NULL" if field in ("points", "grid_idx") else f"{field} is NULL"
            assert _call(name, a) == -3 and msg in _err(), (name, field, _err())
    # what an entry point does not use may be NULL: its checks are passed, and the first one that fails is another
    a = _args(vec_channels=8)
    a.vectors = a.grad_points = None
    assert _call("lp_point_gather", a) == -1 and "channels 8" in _err()
    a = _args(vec_channels=8)
    a.out_features = a.grad_points = None
    assert _call("lp_point_splat", a) == -1 and "channels 8" in _err()
    # the normalisation divides every grid by its weights
    a = _args()
    a.row_weight[1] = None
    assert _call("lp_point_normalize", a) == -3 and "row_weight is NULL for 1 of 3 grids" in _err()
    assert _call("lp_point_normalize", _args(weights=False)) == -3 and "3 of 3 grids" in _err()


def test_malformed_arguments_are_refused():
    for name in ENTRIES:
        assert _call(name, _args(n_rays=-1)) == -1 and "< 0" in _err(), name
        assert _call(name, _args(n_pts=-2)) == -1 and "< 0" in _err()
        assert _call(name, _args(n_rays=1 << 31, n_pts=1 << 31)) == -2 and "wavefronts" in _err()
        # channel mismatch between the per-point vectors and the grids
        assert _call(name, _args(vec_channels=32)) == -1 and "channels 32 of the per-point vectors != grid channels 16" in _err()
        # n_grids / channels out of range
        for n in (0, -1, 9):
            a = _args()
            a.grid.n_grids = n
            assert _call(name, a) == -1 and ("empty grid-list" in _err() or "n_grids" in _err()), (name, n)
        assert _call(name, _args(channels=0)) == -2 and "channels" in _err()
        assert _call(name, _args(channels=129)) == -2 and "129 channels" in _err()
        assert _call(name, _args(channels=128, n_rays=0)) == 0, _err()
        # the grid-list limits are the samplers'
        assert _call(name, _args(sizes=((2, 1, 1, 7),))) == -1 and "non-singular" in _err()
        assert _call(name, _args(sizes=((2, 6, 5, 7), (3, 1, 5, 7)))) == -1 and "batch 3 != 2" in _err()
        a = _args()
        a.grid.n_rows -= 1
        assert _call(name, a) == -1 and "outside the flat tensor" in _err()
    # weights for every grid or for none
    a = _args()
    a.row_weight[2] = None
    assert _call("lp_point_splat", a) == -1 and "row_weight given for 2 of 3 grids" in _err()


def test_under_aligned_pointers_are_refused():
    for name in ENTRIES:
        for off in (4, 8, 2):
            for field in ("points", "grid_idx", "vectors", "out_features", "grad_points"):
                a = _args()
                setattr(a, field, FAKE + 7 * STEP + off)
                assert _call(name, a) == -1 and field in _err() and "16-byte aligned" in _err(), (name, field, off)
            a = _args()
            a.grid.data = FAKE + off
            assert _call(name, a) == -1 and "grid.data" in _err() and "16-byte aligned" in _err()
            a = _args()
            a.grid.grids[1].data = FAKE + 0x100000 + off
            assert _call(name, a) == -1 and "grid.grids[1].data" in _err() and "16-byte aligned" in _err()
            a = _args()
            a.row_weight[2] = FAKE + STEP + off
            assert _call(name, a) == -1 and "row_weight[2]" in _err() and "16-byte aligned" in _err()


def test_wrappers_reject_bad_arguments():
    g = torch.zeros(2, 3, 4, 5, 8)
    sizes = [list(g.shape)]
    pts, idx, feat = torch.zeros(3, 5, 3), torch.zeros(3, dtype=torch.long), torch.zeros(3, 5, 8)
    sample, splat = lp.sample_grid_at_points, lp.splat_points
    for bad in (torch.zeros(3, 5, 2), torch.zeros(15, 3), None):
        with pytest.raises(AssertionError, match=r"\[n_rays, n_pts, 3\]"):
            sample(bad, [g], idx)
        with pytest.raises(AssertionError, match=r"\[n_rays, n_pts, 3\]"):
            splat(bad, feat, sizes, idx)
    for bad in (torch.zeros(4, dtype=torch.long), torch.zeros(3, 1, dtype=torch.long), None):
        with pytest.raises(AssertionError, match="ray_grid_idx"):
            sample(pts, [g], bad)
        with pytest.raises(AssertionError, match="ray_grid_idx"):
            splat(pts, feat, sizes, bad)
    with pytest.raises(AssertionError, match="integer dtype"):
        sample(pts, [g], torch.zeros(3))
    for bad in ((g,), "grid", None):
        with pytest.raises(NotImplementedError):
            sample(pts, bad, idx)
    with pytest.raises(AssertionError, match="grid_sizes cannot be None"):
        sample(pts, g.reshape(-1, 8), idx)
    with pytest.raises(AssertionError, match=r"\[B, D, H, W, C\]"):
        sample(pts, [g[0]], idx)
    for bad in (torch.zeros(3, 5, 4), torch.zeros(3, 8), torch.zeros(3, 4, 8), None):  # (a per-ray [R, C] feature is not broadcast)
        with pytest.raises(AssertionError, match="features"):
            splat(pts, bad, sizes, idx)
    with pytest.raises(AssertionError, match="same feature dimensions"):
        splat(pts, feat, sizes + [[2, 1, 4, 5, 4]], idx)
    with pytest.raises(AssertionError, match="float32"):
        sample(pts.double(), [g], idx)
    with pytest.raises(AssertionError, match="float32"):
        sample(pts, [g.double()], idx)
    with pytest.raises(AssertionError, match="float32"):
        splat(pts, feat.half(), sizes, idx)
    with pytest.raises(AssertionError, match="float32"):
        splat(pts.double(), feat, sizes, idx)
    with pytest.raises(AssertionError, match="contiguous"):
        sample(pts, [torch.zeros(2, 3, 4, 8, 5).transpose(3, 4)], idx)
    # the normalised splat has no point gradient
    with pytest.raises(NotImplementedError, match="normalize=False"):
        splat(pts.clone().requires_grad_(True), feat, sizes, idx)
    with pytest.raises(NotImplementedError, match="normalize=False"):
        splat(pts.clone().requires_grad_(True), feat, sizes, idx, normalize=True, return_list=False)
    # there is no CPU path: tensors that pass every check still need a GPU
    with pytest.raises(_lib.LightplaneHipError, match="GPU only"):
        sample(pts, [g], idx)
    with pytest.raises(_lib.LightplaneHipError, match="GPU only"):
        sample(pts, g.reshape(-1, 8), idx, grid_sizes=sizes)
    with pytest.raises(_lib.LightplaneHipError, match="GPU only"):
        splat(pts, feat, sizes, idx)
    with pytest.raises(_lib.LightplaneHipError, match="GPU only"):
        splat(pts.clone().requires_grad_(True), feat, sizes, idx, normalize=False)


def test_the_case_table_is_the_agreed_one():
    assert list(PG.CASES) == ["triplane_c16", "voxel_c32_flat", "voxel_c5_mask", "triplane_c20_contract_mask", "voxel_c128",
                              "mixed_list_c16", "one_point", "one_wave", "one_cell"]
    assert PG.TOL == 1e-4 and PG.MAX_LEFT_OUT == 0.02 and PG.MAX_ZEROED == 0.05 and PG.FACE_EPS == 1e-5 and PG.CELL_EPS == 1e-3


@pytest.mark.parametrize("name", list(PG.CASES))
def test_inputs_are_admissible(name):
    """the conditions on the GPU tests' inputs, from the oracle alone: both caps hold, and what is left is a real test (non-zero
    results and gradients everywhere; points on both sides of every branch the case is about)"""
    c = PG.case(name)
    n = c["left_out"].numel()
    print(f"{name}: {n} points, {c['counts']}, zeroed {int(c['zeroed'].sum())}")
    assert int(c["left_out"].sum()) <= PG.MAX_LEFT_OUT * n, "change the seed"
    assert int(c["zeroed"].sum()) <= PG.MAX_ZEROED * n or n == 1 and not bool(c["zeroed"].any()), "change the seed"
    if c["mask"]:  # (the weights of the normalised splat count every point: tests/point_grid_cases.py)
        assert int(c["left_out"].sum()) == 0, "change the seed"
        if c["contract"]:  # (the contraction maps every point into the box)
            assert int(c["inside"].sum()) == n
        else:
            assert 0 < int(c["inside"].sum()) < n
    for key in ("gather", "gather_up", "gather_up_norm", "d_points_gather", "d_points_splat"):
        assert bool(torch.isfinite(c[key]).all()) and float(c[key].abs().max()) > 0, key
    for key in ("d_grid", "splat_raw", "splat_norm", "weights"):
        for g in c[key]:
            assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, key
    if c["contract"]:  # points on both sides of the contraction's kink
        far = c["pts"].abs().amax(-1) > 1
        assert 0 < int(far.sum()) < n
    if name == "one_cell":  # every point adds to the same 8 rows
        w = c["weights"][0].reshape(-1)
        assert int((w != 0).sum()) == 8 and abs(float(w.sum()) - n) < 1e-9
    assert (c["gidx"].dtype == torch.int32) == (name == PG.INT32_IDX)

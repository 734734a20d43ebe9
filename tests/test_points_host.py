"""CPU tests of the point evaluation's host side: the lp_points_* symbols and the ABI struct, every argument check of the C ABI (each
returns its code and message before anything touches a device), the Python wrappers' input checks, and the admissibility of the GPU
tests' inputs (tests/points_cases.py), computed from the oracle alone."""
import ctypes
import inspect

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib, grids, params, points
from tests import points_cases as PC

FAKE = 0x10000  # 16-byte-aligned non-NULL "device pointers" far from each other: no check dereferences them, and every call below
STEP = 0x1000000  # fails a check (or has no points to launch for)

DIMS_T, DIMS_O, DIMS_C = [16, 32, 32], [32, 32, 1], [32, 32, 16]
TRIPLANE = ((2, 1, 5, 7), (2, 6, 1, 7), (2, 6, 5, 1))


def _grid_list(sizes, channels, base):
    descs, row = [], 0
    for s in sizes:
        descs.append(grids.GridDesc(*s, row))
        row += descs[-1].n_rows
    gl = _lib.make_grid_list(None, descs, channels, row)
    gl.data = base
    return gl


def _args(sizes=TRIPLANE, channels=16, dims_t=DIMS_T, dims_o=DIMS_O, dims_c=DIMS_C, color_sizes=None, n_rays=3, n_pts=5, enc_dim=None,
          scaffold=None):
    a = _lib.LpPointsArgs()
    a.grid = _grid_list(sizes, channels, FAKE)
    if color_sizes is not None:
        a.color_grid = _grid_list(color_sizes, channels, FAKE + STEP)
    a.mlp_params = FAKE + 2 * STEP
    n_t, n_o = params.mlp_numel(dims_t), params.mlp_numel(dims_o)
    a.n_mlp_params = n_t + n_o + params.mlp_numel(dims_c)
    a.trunk, a.opacity, a.color = _lib.make_mlp(dims_t, 0), _lib.make_mlp(dims_o, n_t), _lib.make_mlp(dims_c, n_t + n_o)
    a.color_chn, a.gain = 3, 1.0
    a.points, a.grid_idx, a.encoding = FAKE + 3 * STEP, FAKE + 4 * STEP, FAKE + 5 * STEP
    a.encoding_dim = (dims_c[0] if dims_c else 0) if enc_dim is None else enc_dim
    a.n_rays, a.n_pts = n_rays, n_pts
    if scaffold is not None:
        a.scaffold = FAKE + 6 * STEP
        a.scaffold_shape = _lib.LpGrid(*scaffold, 0, None)
    a.opacity_out, a.color_out = FAKE + 7 * STEP, FAKE + 8 * STEP
    a.grad_opacity, a.grad_color = FAKE + 9 * STEP, FAKE + 10 * STEP
    return a


def _err():
    return _lib.lib().lp_last_error().decode()


def _fwd(a):
    return _lib.lib().lp_points_forward(ctypes.byref(a), None)


def _bwd(a):
    return _lib.lib().lp_points_backward(ctypes.byref(a), None)


CALLS = (_fwd, _bwd)
TWO_GRID = dict(dims_t=[], dims_o=[16, 32, 1], dims_c=[16, 32, 16], color_sizes=TRIPLANE)


def test_symbols_struct_build_info_and_exports():
    L = _lib.lib()
    for name in ("lp_points_forward", "lp_points_backward"):
        assert hasattr(L, name), f"{name} not exported by liblightplane_hip.so"
        assert name in _lib.EXPORTS
    assert L.lp_abi_sizeof(10) == ctypes.sizeof(_lib.LpPointsArgs)
    assert L.lp_abi_sizeof(9) == -1 and L.lp_abi_sizeof(11) == -1
    assert L.lp_abi_sizeof(8) == ctypes.sizeof(_lib.LpScaffoldArgs)
    assert L.lp_version() == 207  # additive: no version change
    info = _lib.build_info()
    assert "points" in info and "no scratch" in info["points"]["forward"] and "recompute" in info["points"]["backward"]
    assert "scaffold" in info and "grid_resample" in info and "grid_tv" in info  # (its neighbours are still there)
    for name in ("lightplane_eval_mlp", "lightplane_eval_mlp_opacity_only"):
        assert name in lp.__all__ and getattr(lp, name) is getattr(points, name)


def test_signatures_are_the_references():
    sig = inspect.signature(lp.lightplane_eval_mlp)
    assert list(sig.parameters) == ["points", "grid", "ray_grid_idx", "decoder_params", "rays_encoding", "gain",
                                    "mask_out_of_bounds_samples", "inject_opacity_noise", "scaffold", "color_grid", "contract_coords",
                                    "grid_sizes", "color_grid_sizes"]
    assert sig.parameters["grid_sizes"].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(lp.lightplane_eval_mlp_opacity_only)
    assert list(sig.parameters) == ["points", "grid", "ray_grid_idx", "decoder_params", "gain", "mask_out_of_bounds_samples",
                                    "inject_opacity_noise", "scaffold", "contract_coords", "grid_sizes"]
    sig = inspect.signature(lp.LightplaneRenderer.eval_decoder_at_points)
    assert list(sig.parameters)[:11] == ["self", "pts", "pts_to_grid_idx", "rays_encoding", "feature_grid", "color_feature_grid", "scaffold",
                                         "gain", "mask_out_of_bounds_samples", "contract_coords", "directions"]
    assert sig.parameters["grid_sizes"].default is None and sig.parameters["color_grid_sizes"].default is None


def test_well_formed_arguments_without_points_pass():
    """every check passes and nothing is launched: the calls return LP_OK without a device"""
    for call in CALLS:
        assert call(_args(n_rays=0)) == 0, (call.__name__, _err())
        assert call(_args(n_pts=0)) == 0, (call.__name__, _err())
        assert call(_args(n_rays=0, **TWO_GRID)) == 0, (call.__name__, _err())
        assert call(_args(n_rays=0, scaffold=(2, 5, 4, 6))) == 0, (call.__name__, _err())
    # opacity only: no colour result / no colour gradient -> the colour MLP, the encoding and the colour grids are not looked at
    a = _args(n_rays=0, dims_c=[])
    a.color_out = a.grad_color = a.encoding = None
    assert _fwd(a) == 0 and _bwd(a) == 0, _err()
    a = _args(n_rays=0, enc_dim=7)
    a.color_out = a.grad_color = None
    assert _fwd(a) == 0 and _bwd(a) == 0, _err()


def test_null_arguments_are_refused():
    L = _lib.lib()
    assert L.lp_points_forward(None, None) == -3 and "args is NULL" in _err()
    assert L.lp_points_backward(None, None) == -3 and "args is NULL" in _err()
    for call in CALLS:
        for field, msg in (("mlp_params", "mlp_params is NULL"), ("points", "points / grid_idx is NULL"),
                           ("grid_idx", "points / grid_idx is NULL"), ("encoding", "encoding is NULL")):
            a = _args()
            setattr(a, field, None)
            assert call(a) == -3 and msg in _err(), (call.__name__, field, _err())
        a = _args()
        a.grid.data = None  # neither a flat tensor nor per-grid pointers
        assert call(a) == -3 and "grid.data is NULL" in _err()
        a = _args(**TWO_GRID)
        a.color_grid.data = None
        assert call(a) == -3 and "color_grid.data is NULL" in _err()
    a = _args()
    a.opacity_out = None
    assert _fwd(a) == -3 and "opacity_out is NULL" in _err()
    a.n_rays = 0
    assert _bwd(a) == 0, _err()  # (the backward does not look at the forward's results; no points: nothing is launched)


def test_negative_counts_and_too_many_points_are_refused():
    for call in CALLS:
        assert call(_args(n_rays=-1)) == -1 and "< 0" in _err()
        assert call(_args(n_pts=-2)) == -1 and "< 0" in _err()
        assert call(_args(n_rays=1 << 31, n_pts=1 << 31)) == -2 and "wavefronts" in _err()


def test_grid_list_limits_are_the_samplers():
    for call in CALLS:
        assert call(_args(sizes=((2, 1, 1, 7),))) == -1 and "non-singular" in _err(), call.__name__
        assert call(_args(sizes=((2, 6, 5, 7), (3, 1, 5, 7)))) == -1 and "batch 3 != 2" in _err()
        a = _args()
        a.grid.n_grids = 0
        assert call(a) == -1 and "empty grid-list" in _err()
        assert call(_args(channels=129, dims_t=[129, 32, 32])) == -2 and "channels" in _err()


def test_batch_mismatches_are_refused():
    other_batch = tuple((3,) + s[1:] for s in TRIPLANE)
    for call in CALLS:
        assert call(_args(**{**TWO_GRID, "color_sizes": other_batch})) == -1 and "share batch size and channel count" in _err()
        assert call(_args(scaffold=(3, 5, 4, 6))) == -1 and "incompatible with grid batch 2" in _err()
        assert call(_args(scaffold=(2, 5, 0, 6))) == -1 and "scaffold shape" in _err()
        a = _args(**TWO_GRID)
        a.color_grid.channels = 32
        assert call(a) == -1 and "share batch size and channel count" in _err()


def test_decoders_that_do_not_chain_are_refused():
    for call in CALLS:
        assert call(_args(dims_t=[32, 32, 32])) == -1 and "trunk MLP input width 32 != grid channels 16" in _err(), call.__name__
        assert call(_args(dims_o=[16, 32, 1])) == -1 and "opacity MLP input width 16 != 32" in _err()
        assert call(_args(dims_o=[32, 32, 2])) == -1 and "must end in 1 output" in _err()
        assert call(_args(dims_c=[16, 32, 16])) == -1 and "colour MLP input width 16 != 32" in _err()
        assert call(_args(dims_o=[])) == -1 and "opacity MLP has no layers" in _err()
        assert call(_args(dims_c=[])) == -1 and "color MLP has no layers" in _err()  # (the colour head runs: it has to exist)
        assert call(_args(dims_t=[16, 200, 32])) == -2 and "width 200" in _err()
        # the two-grid decoder has no trunk
        assert call(_args(color_sizes=TRIPLANE)) == -1 and "0 layers with a separate colour grid-list" in _err()
        # the encoding is added to the colour head's input
        assert call(_args(enc_dim=16)) == -1 and "encoding_dim 16 != the colour head's input width 32" in _err()
        a = _args()
        a.color_chn = 17
        assert call(a) == -1 and "color_chn 17 outside [1, 16]" in _err()
        a.color_chn = 0
        assert call(a) == -1 and "color_chn 0" in _err()
        for field in ("opacity", "color"):
            a = _args()
            getattr(a, field).offset += 1
            assert call(a) == -1 and "flat layout" in _err()
        a = _args()
        a.n_mlp_params -= 1
        assert call(a) == -1 and "mlp_params has" in _err()


def test_under_aligned_pointers_are_refused():
    fields = ("mlp_params", "points", "grid_idx", "encoding", "opacity_out", "color_out", "grad_opacity", "grad_color", "grad_grid",
              "grad_color_grid", "grad_mlp_params", "grad_encoding", "grad_points")
    for call in CALLS:
        for off in (4, 8, 2):
            for field in fields:
                a = _args()
                setattr(a, field, FAKE + 11 * STEP + off)
                assert call(a) == -1 and field in _err() and "16-byte aligned" in _err(), (call.__name__, field, off)
            a = _args(scaffold=(2, 5, 4, 6))
            a.scaffold = FAKE + 6 * STEP + off
            assert call(a) == -1 and "scaffold" in _err() and "16-byte aligned" in _err()
            a = _args()
            a.grid.data = FAKE + off
            assert call(a) == -1 and "grid.data" in _err() and "16-byte aligned" in _err()
            a = _args()
            a.grid.grids[1].data = FAKE + 0x100000 + off
            assert call(a) == -1 and "grid.grids[1].data" in _err() and "16-byte aligned" in _err()
            a = _args(**TWO_GRID)
            a.color_grid.grids[2].data = FAKE + STEP + 0x100000 + off
            assert call(a) == -1 and "color_grid.grids[2].data" in _err() and "16-byte aligned" in _err()
            a = _args()
            a.grad_grid_list[2] = FAKE + 12 * STEP + off
            assert call(a) == -1 and "grad_grid_list[2]" in _err() and "16-byte aligned" in _err()
            a = _args(**TWO_GRID)
            a.grad_color_grid_list[0] = FAKE + 12 * STEP + off
            assert call(a) == -1 and "grad_color_grid_list[0]" in _err() and "16-byte aligned" in _err()


def test_backward_only_checks():
    # gradient buffers for every grid of a list or for none
    a = _args()
    a.grad_grid_list[0] = FAKE + 12 * STEP
    assert _bwd(a) == -1 and "given for 1 of 3 grids" in _err()
    # layer widths summing beyond the private activation array
    wide = [128] * 5
    a = _args(channels=128, dims_t=wide, dims_o=[128, 128, 128, 1], dims_c=[128, 128, 128, 16], sizes=((2, 4, 3, 5),))
    assert _bwd(a) == -2 and "exceeds 1024" in _err()
    a.n_rays = 0
    assert _fwd(a) == 0, _err()  # (the forward keeps nothing per layer: any depth)


def _decoder():
    return lp.init_decoder_params(device="cpu", n_layers_opacity=2, n_layers_trunk=2, n_layers_color=2, input_chn=8, hidden_chn=16,
                                  color_chn=3)


def test_wrappers_reject_bad_arguments():
    dec = _decoder()
    g = torch.zeros(2, 3, 4, 5, 8)
    pts, idx, enc = torch.zeros(3, 5, 3), torch.zeros(3, dtype=torch.long), torch.zeros(3, 16)
    joint = lambda *a, **k: lp.lightplane_eval_mlp(*a, **k)  # noqa: E731
    with pytest.raises(NotImplementedError, match="inject_opacity_noise"):
        lp.lightplane_eval_mlp(pts, [g], idx, dec, enc, 1.0, False, torch.zeros(3, 5))
    with pytest.raises(NotImplementedError, match="inject_opacity_noise"):
        lp.lightplane_eval_mlp_opacity_only(pts, [g], idx, dec, 1.0, inject_opacity_noise=torch.zeros(3, 5))
    for bad in (torch.zeros(3, 5, 2), torch.zeros(15, 3), None):
        with pytest.raises(AssertionError, match=r"\[n_rays, n_pts, 3\]"):
            joint(bad, [g], idx, dec, enc, 1.0)
    with pytest.raises(AssertionError, match="ray_grid_idx"):
        joint(pts, [g], torch.zeros(4, dtype=torch.long), dec, enc, 1.0)
    for bad in (torch.zeros(3, 8), torch.zeros(4, 16), None):
        with pytest.raises(AssertionError, match="rays_encoding"):
            joint(pts, [g], idx, dec, bad, 1.0)
    for bad in ((g,), "grid", None):
        with pytest.raises(NotImplementedError):
            joint(pts, bad, idx, dec, enc, 1.0)
    with pytest.raises(AssertionError, match="grid_sizes cannot be None"):
        joint(pts, g.reshape(-1, 8), idx, dec, enc, 1.0)
    with pytest.raises(AssertionError, match="same type"):
        joint(pts, [g], idx, dec, enc, 1.0, color_grid=g.reshape(-1, 8), color_grid_sizes=[list(g.shape)])
    with pytest.raises(AssertionError, match="no trunk layers"):
        joint(pts, [g], idx, dec, enc, 1.0, color_grid=[g])
    with pytest.raises(AssertionError, match="float32"):
        joint(pts.double(), [g], idx, dec, enc, 1.0)
    with pytest.raises(AssertionError, match="float32"):
        joint(pts, [g.double()], idx, dec, enc, 1.0)
    with pytest.raises(AssertionError, match="contiguous"):
        joint(pts, [torch.zeros(2, 3, 4, 8, 5).transpose(3, 4)], idx, dec, enc, 1.0)
    with pytest.raises(AssertionError, match=r"\[B, D, H, W\]"):
        joint(pts, [g], idx, dec, enc, 1.0, scaffold=torch.zeros(3, 4, 5))
    # there is no CPU path: tensors that pass every check still need a GPU
    with pytest.raises(_lib.LightplaneHipError, match="GPU only"):
        joint(pts, [g], idx, dec, enc, 1.0)
    with pytest.raises(_lib.LightplaneHipError, match="GPU only"):
        lp.lightplane_eval_mlp_opacity_only(pts, g.reshape(-1, 8), idx, dec, 1.0, grid_sizes=[list(g.shape)])


def test_module_routing_needs_gpu_tensors():
    """tensors that are not fp32 on a GPU never reach the fused functions: the Renderer path then raises what it always raised"""
    from lightplane_amd.modules import _fused_points_supported
    g = torch.zeros(1, 1, 4, 4, 16)
    pts = torch.zeros(2, 3, 3)
    assert not _fused_points_supported(pts, [g]) and not _fused_points_supported(pts.double(), [g])
    assert not _fused_points_supported(None, [g]) and not _fused_points_supported(pts, [])
    assert not _fused_points_supported(pts, [g], color_feature_grid=g.reshape(-1, 16))


@pytest.mark.parametrize("name", list(PC.CASES))
def test_inputs_are_admissible(name):
    """the conditions on the GPU tests' inputs, from the oracle alone: few points are left out of the value comparison, few have their
    upstream gradient zeroed, and what is left is a real test (non-zero results and gradients everywhere)"""
    c = PC.case(name)
    n = c["left_out"].numel()
    print(f"{name}: {n} points, {c['counts']}, zeroed {int(c['zeroed'].sum())}")
    assert int(c["left_out"].sum()) <= PC.MAX_LEFT_OUT * n or n == 1 and not bool(c["left_out"].any()), "change the seed"
    assert int(c["zeroed"].sum()) <= PC.MAX_ZEROED * n or n == 1 and not bool(c["zeroed"].any()), "change the seed"
    assert bool(torch.isfinite(c["op"]).all()) and bool(torch.isfinite(c["col"]).all())
    assert float(c["op"].abs().max()) > 0 and float(c["col"].abs().max()) > 0
    gr = c["grads"]
    for key in ("points", "params", "enc"):
        assert bool(torch.isfinite(gr[key]).all()) and float(gr[key].abs().max()) > 0, key
    for g in gr["grids"] + (gr["cgrids"] or []):
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    if c["scaffold"] is not None:  # the scaffold removes some points and keeps others
        occ = c["op"] == 0
        assert 0 < int(occ.sum()) < n
    if c["contract"]:  # points on both sides of the contraction's kink
        far = c["pts"].abs().amax(-1) > 1
        assert 0 < int(far.sum()) < n

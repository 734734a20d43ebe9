"""CPU tests of the host side of ``kplanes_eval_mlp``: the exclusion caps of tests/kplanes_points_cases.py from its fp64 reference, the
wrapper's errors, and the C-ABI checks (before anything touches a device)."""
import ctypes
import json

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib, kplanes
from tests import kplanes_points_cases as KC
from tests.synth import random_decoder

FAKE, STEP = 0x10000, 0x1000000  # 16-byte-aligned non-NULL "device pointers": no check dereferences them
EXPORTS = ("lp_kplanes_points_forward", "lp_kplanes_points_backward")
POINTERS = ("planes", "grad_planes", "points", "times", "grid_idx", "mlp_params", "encoding", "scaffold", "opacity_out", "color_out",
            "grad_opacity", "grad_color", "grad_mlp_params", "grad_encoding", "grad_points")


def _decoder(width, n_t=2):
    return random_decoder(torch.Generator().manual_seed(5), n_t, 2, 2, width, 32, 3)


def _args(n_rays=3, n_pts=70, dec=None):
    lay = lp.kplanes_layout(**KC.DYN)
    dec = dec or _decoder(lay.out_channels)
    dims = [tuple(kplanes.int_list_of(v)) for v in (dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color)]
    cfg = kplanes._EvalCfg(kplanes._Cfg(lay, False, False), *dims, 3, 1.0, False)
    a = kplanes._eval_args(cfg, torch.zeros(1, 1, 3), torch.zeros(1), torch.zeros(2, 1, 1), dec.mlp_params, torch.zeros(1, dims[2][0]),
                           torch.zeros(1), torch.zeros(2, 5, 4, 6), True)
    a.n_rays, a.n_pts = n_rays, n_pts
    for i, f in enumerate(POINTERS):
        setattr(a, f, FAKE + i * STEP)
    return a


_err = lambda: _lib.lib().lp_last_error().decode()  # noqa: E731
_call = lambda name, a: getattr(_lib.lib(), name)(ctypes.byref(a), None)  # noqa: E731


@pytest.mark.parametrize("name", KC.ALL)
def test_exclusion_caps_hold(name):
    c = KC.case(name)
    n, zeroed, left = c["zeroed"].numel(), int(c["zeroed"].sum()), int(c["left_out"].sum())
    print(f"{name}: {n} points, {zeroed} with a zero upstream gradient, {left} left out, {int((~c['inside']).sum())} masked, "
          f"{int((c['occ'] == 0).sum())} with occ = 0")
    assert zeroed <= KC.MAX_ZEROED * n and left <= KC.MAX_LEFT_OUT * n
    assert float(c["op"].abs().max()) > 0.1 and all(float(g.abs().max()) > 0 for g in c["grads"].values())
    assert name != "contract_mask_scaffold" or 0 < int((c["occ"] == 0).sum()) < n
    assert name != "masked_112x32" or 0 < int(c["inside"].sum()) < n


def test_wrapper_errors():
    assert lp.kplanes_eval_mlp is kplanes.kplanes_eval_mlp and lp.kplanes_eval_mlp_opacity_only is kplanes.kplanes_eval_mlp_opacity_only
    lay, static = lp.kplanes_layout(**KC.DYN), lp.kplanes_layout(**dict(KC.DYN, time_resolution=None))
    planes, dec = lp.init_kplanes(lay, 2), _decoder(lay.out_channels)
    pts, idx, enc, times = torch.zeros(3, 5, 3), torch.zeros(3, dtype=torch.int64), torch.zeros(3, 32), torch.zeros(3)
    with pytest.raises(ValueError, match="the decoder reads 8 features, the layout has n_scales x channels = 16"):
        lp.kplanes_eval_mlp_opacity_only(pts, times, planes, idx, lay, _decoder(8), 1.0)
    with pytest.raises(ValueError, match="times has to be a tensor for a dynamic layout"):
        lp.kplanes_eval_mlp(pts, None, planes, idx, lay, dec, enc, 1.0)
    with pytest.raises(ValueError, match="times has to be None for a static layout"):
        lp.kplanes_eval_mlp(pts, times, lp.init_kplanes(static, 2), idx, static, dec, enc, 1.0)
    with pytest.raises(NotImplementedError, match="times requires a gradient"):
        lp.kplanes_eval_mlp(pts, times.clone().requires_grad_(True), planes, idx, lay, dec, enc, 1.0)
    with pytest.raises(ValueError, match=rf"planes has to be a \[B, {lay.rows}, 8\]"):
        lp.kplanes_eval_mlp(pts, times, planes[:, :-1], idx, lay, dec, enc, 1.0)
    with pytest.raises(_lib.LightplaneHipError, match="GPU only"):   # there is no CPU path
        lp.kplanes_eval_mlp(pts, times, planes, idx, lay, dec, enc, 1.0)


@pytest.mark.parametrize("name", EXPORTS)
def test_abi_refusals(name):
    L = _lib.lib()
    assert _lib.KPLANES_POINTS_EXPORTS == EXPORTS and L.lp_abi_sizeof(54) == ctypes.sizeof(_lib.LpKPlanesPointsArgs)
    assert [L.lp_abi_sizeof(w) for w in (52, 53, 55)] == [-1, -1, -1]
    assert set(json.loads(L.lp_build_info().decode())["points"]["kplanes_points"]) == {"forward", "backward"}
    assert getattr(L, name)(None, None) == -3 and "args is NULL" in _err()
    for f in ("planes", "points", "mlp_params") + (("opacity_out",) if name == EXPORTS[0] else ()):
        a = _args()
        setattr(a, f, None)
        assert _call(name, a) == -3 and _err().startswith(f"{f} is NULL"), (f, _err())
    a = _args()
    a.grad_planes = FAKE + 4
    assert _call(name, a) == -1 and _err().startswith("grad_planes = ") and "16-byte aligned" in _err(), _err()
    a = _args()
    a.offset[1][0] = 3   # a broken layout: the rules are those of lp_kplanes_*
    assert _call(name, a) == -1 and "offset[1][0]" in _err(), _err()
    a = _args()
    a.n_scales = 1       # the trunk reads S * C features
    assert _call(name, a) == -1 and "trunk MLP input width 16 != grid channels 8" in _err(), _err()
    assert _call(name, _args(dec=_decoder(32, 0))) == -1 and "opacity MLP input width 32 != 16" in _err(), _err()
    for n_rays, n_pts in ((0, 70), (3, 0)):   # an empty batch passes every check and launches nothing
        assert _call(name, _args(n_rays=n_rays, n_pts=n_pts)) == 0, _err()

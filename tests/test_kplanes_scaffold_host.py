"""CPU tests of the host side of the plane-field scaffold: the occupancy thresholds of tests/kplanes_scaffold_cases.py from its fp64
reference, the wrapper's errors, and the C-ABI checks (before anything touches a device)."""
import ctypes
import json

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib, kplanes_scaffold
from tests import kplanes_scaffold_cases as SC
from tests.synth import random_decoder
from tests.test_gpu_scaffold import GAP

FAKE, STEP = 0x10000, 0x1000000  # 16-byte-aligned non-NULL "device pointers": no check dereferences them
EXPORTS = ("lp_kplanes_scaffold_workspace_bytes", "lp_kplanes_scaffold_opacity", "lp_kplanes_scaffold_build")
_err = lambda: _lib.lib().lp_last_error().decode()  # noqa: E731


def _decoder(width, n_t=2, hidden=32):
    return random_decoder(torch.Generator().manual_seed(5), n_t, 2, 2, width, hidden, 3)


def _args(dec=None, layout=SC.KP.DYN, size=(2, 3, 4, 70)):
    lay = lp.kplanes_layout(**layout)
    a = _lib.LpKPlanesScaffoldArgs()
    a.planes, a.times, a.mlp_params = FAKE, (FAKE + STEP if lay.n_planes == 6 else None), FAKE + 2 * STEP
    a.n_times, a.batch, a.rows = 3, 2, lay.rows
    a.channels, a.n_scales, a.n_planes = lay.channels, lay.n_scales, lay.n_planes
    for s in range(lay.n_scales):
        a.spatial[s], a.temporal[s] = lay.spatial[s], lay.temporal[s] if lay.temporal else 0
        for j in range(lay.n_planes):
            a.offset[s][j] = lay.offsets[s][j]
    dec = dec or _decoder(lay.out_channels)
    a.n_mlp_params = dec.mlp_params.numel()
    _lib.make_decoder(a, *(tuple(kplanes_scaffold.int_list_of(v)) for v in (dec.n_hidden_trunk, dec.n_hidden_opacity)))
    a.gain, a.threshold, a.dilate, a.shape = 1.0, 0.5, 1, _lib.LpGrid(*size, 0, None)
    return a


def _call(name, a, out=FAKE + 3 * STEP):
    L = _lib.lib()
    if name == EXPORTS[1]:
        return L.lp_kplanes_scaffold_opacity(ctypes.byref(a), out, None)
    return L.lp_kplanes_scaffold_build(ctypes.byref(a), out, FAKE + 4 * STEP, 1 << 20, None)


@pytest.mark.parametrize("name", SC.ALL)
def test_thresholds_are_unambiguous(name):
    c = SC.case(name)
    print(f"{name}: threshold {c['t']:.6g}, gap {c['gap']:.3e} of max |opacity| {float(c['op'].abs().max()):.4g}")
    assert c["gap"] > GAP, f"{name}: widest gap {c['gap']:.3e} <= {GAP}: change the seed"
    assert 0 < float((c["op"] > c["t"]).float().mean()) < 1 or c["op"].numel() < 4


def test_wrapper_errors():
    lay, static = lp.kplanes_layout(**SC.KP.DYN), lp.kplanes_layout(**dict(SC.KP.DYN, time_resolution=None))
    planes, dec, times = lp.init_kplanes(lay, 2), _decoder(lay.out_channels), torch.zeros(3)
    for fn in (lp.kplanes_scaffold_opacity, lp.kplanes_calculate_scaffold):
        with pytest.raises(ValueError, match="times has to be None for a static layout"):
            fn(lp.init_kplanes(static, 2), static, dec, (2, 3, 4, 5), times=times)
        with pytest.raises(ValueError, match="times has to be a 1-D tensor"):
            fn(planes, lay, dec, (2, 3, 4, 5))
        with pytest.raises(ValueError, match=r"scaffold_size\[0\] = 1 has to be the batch size 2"):
            fn(planes, lay, dec, (1, 3, 4, 5), times=times)
        with pytest.raises(ValueError, match="the decoder reads 8 features, the layout has n_scales x channels = 16"):
            fn(planes, lay, _decoder(8), (2, 3, 4, 5), times=times)
        with pytest.raises(_lib.LightplaneHipError, match="GPU only"):   # there is no CPU path
            fn(planes, lay, dec, (2, 3, 4, 5), times=times)
    assert lp.kplanes_scaffold_workspace_bytes((2, 3, 4, 5), 2) == 120 and lp.kplanes_scaffold_workspace_bytes((2, 3, 4, 5), 0) == 0


@pytest.mark.parametrize("name", EXPORTS[1:])
def test_abi_refusals(name):
    L = _lib.lib()
    assert _lib.KPLANES_SCAFFOLD_EXPORTS == EXPORTS and L.lp_abi_sizeof(66) == ctypes.sizeof(_lib.LpKPlanesScaffoldArgs)
    assert [L.lp_abi_sizeof(w) for w in (64, 65, 67)] == [-1, -1, -1]
    assert set(json.loads(L.lp_build_info().decode())["points"]["kplanes_scaffold"]) == {"lattice", "dilation"}
    assert getattr(L, name)(None, *((None, None) if name == EXPORTS[1] else (None, None, 0, None))) == -3 and "args is NULL" in _err()
    for f in ("planes", "times", "mlp_params"):   # (NULL times with six planes)
        a = _args()
        setattr(a, f, None)
        assert _call(name, a) == -3 and _err().startswith(f"{f} is NULL"), (f, _err())
    assert _call(name, _args(), out=None) == -3 and "result pointer is NULL" in _err(), _err()
    a = _args()
    a.times = FAKE + 4
    assert _call(name, a) == -1 and _err().startswith("times = ") and "16-byte aligned" in _err(), _err()
    a = _args()
    a.offset[1][0] = 3   # a broken layout: the rules are those of lp_kplanes_*
    assert _call(name, a) == -1 and "offset[1][0]" in _err(), _err()
    a = _args(layout=dict(SC.KP.DYN, time_resolution=None))
    a.times = FAKE + STEP
    assert _call(name, a) == -1 and "times given for a static layout" in _err(), _err()
    a = _args()
    a.n_scales = 1       # the trunk reads S * C features
    assert _call(name, a) == -1 and "trunk MLP input width 16 != grid channels 8" in _err(), _err()
    assert _call(name, _args(dec=_decoder(32, 0))) == -1 and "opacity MLP input width 32 != 16" in _err(), _err()
    a = _args()
    a.n_mlp_params = 100   # (fewer than trunk and opacity head take)
    assert _call(name, a) == -1 and "mlp_params has" in _err(), _err()
    assert _call(name, _args(size=(1, 3, 4, 70))) == -1 and "scaffold batch 1 != batch 2" in _err(), _err()
    assert _call(name, _args(size=(2, 3, 0, 70))) == -1 and "extent < 1" in _err(), _err()
    a = _args()
    a.n_times = 0
    assert _call(name, a) == -1 and "n_times 0 < 1" in _err(), _err()
    a = _args()
    a.channels = 12
    assert _call(name, a) == -2 and "channels 12" in _err(), _err()
    assert _call(name, _args(dec=_decoder(16, hidden=129))) == -2 and "width 129" in _err(), _err()
    a = _args(size=(2, 1024, 1024, 1024))
    assert _call(name, a) == -2 and "2^31 points or more" in _err(), _err()
    assert L.lp_kplanes_scaffold_workspace_bytes(ctypes.byref(a)) == -2
    if name == EXPORTS[2]:   # the workspace rule of lp_scaffold_build
        assert L.lp_kplanes_scaffold_build(ctypes.byref(_args()), FAKE, None, 0, None) == -1 and "workspace is NULL" in _err(), _err()
        assert L.lp_kplanes_scaffold_build(ctypes.byref(_args()), FAKE, FAKE + STEP, 100, None) == -1 and "asks for 1680" in _err(), _err()
        assert L.lp_kplanes_scaffold_build(ctypes.byref(_args()), FAKE, FAKE + 16, 1 << 20, None) == -1 and "overlaps" in _err(), _err()

"""CPU tests of the host side of ``kplanes_encode``: symbols, ABI struct and header, every refusal class (before anything touches a device),
the layout against hand-computed tables, the initialisation, the wrapper's errors, and the exclusion caps of tests/test_gpu_kplanes.py's
cases from its fp64 reference."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib, kplanes
from tests import test_gpu_kplanes as KP

FAKE, STEP = 0x10000, 0x1000000  # 16-byte-aligned non-NULL "device pointers": no check dereferences them
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lightplane_hip_kplanes.h")
EXPORTS = ("lp_kplanes_forward", "lp_kplanes_backward_planes", "lp_kplanes_backward_points")
POINTERS = ("planes", "grad_planes", "points", "times", "grid_idx", "out_features", "grad_features", "grad_points")
NEEDED = {EXPORTS[0]: ("points", "grid_idx", "times", "planes", "out_features"),
          EXPORTS[1]: ("points", "grid_idx", "times", "planes", "grad_features", "grad_planes"),
          EXPORTS[2]: ("points", "grid_idx", "times", "planes", "grad_features", "grad_points")}


def _args(n_rays=3, n_pts=70, **layout):
    lay = lp.kplanes_layout(**(layout or KP.DYN))
    a = kplanes._args(kplanes._Cfg(lay, False, False), torch.zeros(1, 1, 3), None, torch.zeros(1), 2)
    a.n_rays, a.n_pts = n_rays, n_pts
    for i, f in enumerate(POINTERS):
        setattr(a, f, FAKE + i * STEP if f != "times" or lay.n_planes == 6 else None)
    return a


_err = lambda: _lib.lib().lp_last_error().decode()  # noqa: E731
_call = lambda name, a: getattr(_lib.lib(), name)(ctypes.byref(a), None)  # noqa: E731


def test_symbols_struct_and_header(tmp_path):
    L = _lib.lib()
    text = open(HEADER).read()
    assert _lib.KPLANES_EXPORTS == EXPORTS == tuple(re.findall(r"^int (lp_\w+)\(", text, re.M))
    assert all(hasattr(L, n) and n not in _lib.EXPORTS + _lib.HASH_GRID_EXPORTS for n in EXPORTS)
    assert L.lp_abi_sizeof(50) == ctypes.sizeof(_lib.LpKPlanesArgs)
    assert [L.lp_abi_sizeof(w) for w in (48, 49, 51)] == [-1, -1, -1] and L.lp_version() == 207
    assert "run merging" in _lib.build_info()["points"]["kplanes"]["backward_planes"]   # (no new top-level key: the text's keys are pinned)
    from lightplane_amd.csrc import build as B
    assert any(h.endswith("lightplane_hip_kplanes.h") for h in B.PUBLIC_HEADERS) and "lp_kplanes.hip" in B.SOURCES
    assert '#include "../../include/lightplane_hip_kplanes.h"' in open(os.path.join(B.HERE, "lp_host.h")).read()
    cc = shutil.which("cc") or shutil.which("gcc")   # (a C compiler is needed: the header has to pass it as plain C)
    src, exe = tmp_path / "sizes.c", tmp_path / "sizes"
    src.write_text('#include <stdio.h>\n#include "lightplane_hip_kplanes.h"\nint main(void){printf("%zu\\n", '
                   'sizeof(LpKPlanesArgs)); return 0;}\n')
    subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert int(subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE).stdout.split()[0]) == L.lp_abi_sizeof(50)


@pytest.mark.parametrize("name", EXPORTS)
def test_refusals(name):
    """each refusal class once per entry point; none reaches a device"""
    assert getattr(_lib.lib(), name)(None, None) == -3 and "args is NULL" in _err()
    for f in NEEDED[name]:
        a = _args()
        setattr(a, f, None)
        assert _call(name, a) == -3 and _err().startswith(f"{f} is NULL"), (f, _err())
    for f in POINTERS:
        a = _args()
        setattr(a, f, FAKE + 4)
        assert _call(name, a) == -1 and _err().startswith(f"{f} = ") and "16-byte aligned" in _err(), (f, _err())

    def bad(code, starts, static=False, **fields):
        a = _args(**(dict(KP.DYN, time_resolution=None) if static else {}))
        for k, v in fields.items():
            if isinstance(v, tuple):
                target = getattr(a, k)
                for i in v[:-2]:
                    target = target[i]
                target[v[-2]] = v[-1]
            else:
                setattr(a, k, v)
        assert _call(name, a) == code and _err().startswith(starts), (fields, _err())

    # DYN: scale 0 has planes of 25, 25, 25, 20, 20, 20 rows from 0; scale 1 of 81, 81, 81, 36, 36, 36 from 135; 486 rows
    bad(-1, "offset[0][1]", offset=(0, 1, 24))        # overlaps the plane before
    bad(-1, "offset[1][0]", offset=(1, 0, 134))       # a scale begins inside the one before
    bad(-1, "offset[1][1]", spatial=(1, 10))          # a finer scale no longer fits its offsets
    bad(-1, "rows", rows=485)                         # the planes end at 486
    bad(-1, "spatial[0]", spatial=(0, 1))
    bad(-1, "spatial[1]", spatial=(1, 4097))
    bad(-1, "temporal[0]", temporal=(0, 1))
    bad(-1, "n_scales", n_scales=9)
    bad(-1, "n_planes 4", n_planes=4)
    bad(-1, "batch", batch=0)
    bad(-1, "time_per_point", time_per_point=2)
    bad(-1, "times given", static=True, times=FAKE)   # a static layout reads no timestamps
    bad(-2, "channels 12", channels=12)
    a = _args(resolutions=(4, 4), time_resolution=3, channels=64)   # (a third scale by hand: kplanes_layout stops at 128 channels)
    a.n_scales, a.spatial[2], a.temporal[2] = 3, 4, 3
    for j in range(6):
        a.offset[2][j] = a.rows + j * 16
    a.rows += 96
    assert _call(name, a) == -2 and "192 channels > 128" in _err(), _err()
    assert _call(name, _args(n_rays=1 << 24, n_pts=128)) == -2 and "2^31" in _err(), _err()
    assert _call(name, _args(n_rays=-1)) == -1
    for n_rays, n_pts in ((0, 70), (3, 0)):   # an empty batch passes every check and launches nothing
        assert _call(name, _args(n_rays=n_rays, n_pts=n_pts)) == 0, _err()


def test_layout_against_hand_computed_tables():
    lay = lp.kplanes_layout((5, 9), (4, 4), 8)
    assert lay == (2, 6, 8, (5, 9), (4, 4), ((0, 25, 50, 75, 95, 115), (135, 216, 297, 378, 414, 450)), 486, 16)
    assert lp.kplanes_layout((5, 9), 4, 8) == lay
    assert lp.kplanes_layout((5, 9), None, 4) == (2, 3, 4, (5, 9), (), ((0, 25, 50), (75, 156, 237)), 318, 8)
    lay = lp.kplanes_layout()                     # the default: four static scales of 32 channels
    assert lay.n_planes == 3 and lay.spatial == (64, 128, 256, 512) and lay.out_channels == 128
    assert lay.rows == 3 * (64 ** 2 + 128 ** 2 + 256 ** 2 + 512 ** 2) and lay.offsets[3][2] == lay.rows - 512 ** 2
    assert lp.kplanes_layout((2,), (4096,), 64)[5:7] == (((0, 4, 8, 12, 8204, 16396),), 24588)
    for kw in (dict(resolutions=()), dict(resolutions=(4,) * 9, channels=4), dict(channels=12), dict(channels=2), dict(channels=128),
               dict(resolutions=(4,) * 5), dict(resolutions=(4, 4, 4), channels=64), dict(resolutions=(1, 8)), dict(resolutions=(8, 4097)),
               dict(time_resolution=1), dict(time_resolution=4097), dict(time_resolution=(4, 4, 4)), dict(time_resolution=(4, 4, 4, 1))):
        with pytest.raises(ValueError):
            lp.kplanes_layout(**kw)


def test_python_surface():
    for name in kplanes.__all__:
        assert name in lp.__all__ and getattr(lp, name) is getattr(kplanes, name)
    lay, static = lp.kplanes_layout(**KP.DYN), lp.kplanes_layout((5, 9), None, 8)
    planes = lp.init_kplanes(lay, 2, low=0.2, high=0.4, generator=torch.Generator().manual_seed(1))
    assert planes.shape == (2, 486, 8) and planes.dtype == torch.float32
    for s, n_space in enumerate((75, 243)):   # space planes inside [low, high], space-time planes all 1
        first = lay.offsets[s][0]
        space, space_time = planes[:, first:first + n_space], planes[:, lay.offsets[s][3]:lay.offsets[s][5] + lay.spatial[s] * 4]
        assert 0.2 <= float(space.min()) < 0.21 and 0.39 < float(space.max()) <= 0.4 and bool((space_time == 1).all())
        assert first + n_space == lay.offsets[s][3]
    assert float(lp.init_kplanes(static, 1, low=0.2, high=0.4).max()) <= 0.4
    pts, idx, times = torch.zeros(3, 5, 3), torch.zeros(3, dtype=torch.int64), torch.zeros(3)
    for wrong in (planes[:, :-8], planes[..., :4], planes[0], torch.zeros(2, 486, 16)):
        with pytest.raises(ValueError, match=r"planes has to be a \[B, 486, 8\]"):
            lp.kplanes_encode(pts, times, wrong, idx, lay)
    with pytest.raises(ValueError, match="layout"):
        lp.kplanes_encode(pts, times, planes, idx, tuple(lay))
    with pytest.raises(ValueError, match="times has to be None"):
        lp.kplanes_encode(pts, times, planes[:, :318], idx, static)
    with pytest.raises(ValueError, match="times has to be a tensor"):
        lp.kplanes_encode(pts, None, planes, idx, lay)
    with pytest.raises(AssertionError, match=r"times has to be a \[3\] or a \[3, 5\]"):
        lp.kplanes_encode(pts, torch.zeros(5), planes, idx, lay)
    with pytest.raises(NotImplementedError, match=r"times\.detach\(\)"):
        lp.kplanes_encode(pts, times.clone().requires_grad_(), planes, idx, lay)
    with pytest.raises(AssertionError, match="planes has to be float32"):
        lp.kplanes_encode(pts, times, planes.double(), idx, lay)
    with pytest.raises(AssertionError, match="integer"):
        lp.kplanes_encode(pts, times, planes, idx.float(), lay)
    for t in (times, torch.zeros(3, 5)):
        with pytest.raises(_lib.LightplaneHipError, match="GPU only"):   # there is no CPU path
            lp.kplanes_encode(pts, t, planes, idx, lay)


@pytest.mark.parametrize("name", KP.ALL)
def test_exclusion_caps_hold(name):
    c = KP.case(name)
    n, zeroed, left = c["zeroed"].numel(), int(c["zeroed"].sum()), int(c["left_out"].sum())
    print(f"{name}: {n} points, {zeroed} without a point gradient, {left} left out (cube face), {int((~c['inside']).sum())} masked")
    assert zeroed <= KP.MAX_ZEROED * n and left <= KP.MAX_LEFT_OUT * n
    assert c["mask"] or left == 0
    assert float(c["d_points"].abs().max()) > 0 and float(c["d_planes"].abs().max()) > 0
    assert name == "min_res" or 0 < int(c["untouched"].sum())   # (one cell per plane: every row is read)
    assert float(c["want"].abs().max()) > 0.1 and bool(torch.isfinite(c["d_planes"]).all())
    assert name != "masked" or 0 < int(c["inside"].sum()) < n

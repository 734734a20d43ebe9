"""CPU tests of the host side of ``hash_grid_encode``: symbols, ABI struct and header, every refusal class (before anything touches a device),
the layout against hand-computed tables, the wrapper's errors, and the exclusion caps of tests/test_gpu_hash_grid.py's cases from its fp64 reference."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib, hash_grid
from tests import test_gpu_hash_grid as HG

FAKE, STEP = 0x10000, 0x1000000  # 16-byte-aligned non-NULL "device pointers": no check dereferences them
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lightplane_hip_hash_grid.h")
EXPORTS = ("lp_hash_grid_forward", "lp_hash_grid_backward_table", "lp_hash_grid_backward_points")
POINTERS = ("table", "grad_table", "points", "grid_idx", "out_features", "grad_features", "grad_points")
NEEDED = {EXPORTS[0]: ("points", "grid_idx", "table", "out_features"), EXPORTS[1]: ("points", "grid_idx", "grad_features", "grad_table"),
          EXPORTS[2]: ("points", "grid_idx", "table", "grad_features", "grad_points")}


def _args(n_rays=3, n_pts=70, **layout):
    a = hash_grid._args(hash_grid._Cfg(lp.hash_grid_layout(**(layout or HG.MIXED)), False, False), torch.zeros(1, 1, 3), torch.zeros(1), 2)
    a.n_rays, a.n_pts = n_rays, n_pts
    for i, f in enumerate(POINTERS):
        setattr(a, f, FAKE + i * STEP)
    return a


_err = lambda: _lib.lib().lp_last_error().decode()  # noqa: E731
_call = lambda name, a: getattr(_lib.lib(), name)(ctypes.byref(a), None)  # noqa: E731


def test_symbols_struct_and_header(tmp_path):
    L = _lib.lib()
    text = open(HEADER).read()
    assert _lib.HASH_GRID_EXPORTS == EXPORTS == tuple(re.findall(r"^int (lp_\w+)\(", text, re.M))
    assert all(hasattr(L, n) and n not in _lib.EXPORTS + _lib.RAY_GRID_EXPORTS for n in EXPORTS)
    assert L.lp_abi_sizeof(38) == ctypes.sizeof(_lib.LpHashGridArgs)
    assert [L.lp_abi_sizeof(w) for w in (36, 37, 39)] == [-1, -1, -1] and L.lp_version() == 207
    from lightplane_amd.csrc import build as B
    assert any(h.endswith("lightplane_hip_hash_grid.h") for h in B.PUBLIC_HEADERS) and "lp_hash_grid.hip" in B.SOURCES
    assert '#include "../../include/lightplane_hip_hash_grid.h"' in open(os.path.join(B.HERE, "lp_host.h")).read()
    cc = shutil.which("cc") or shutil.which("gcc")   # (a C compiler is needed: the header has to pass it as plain C)
    src, exe = tmp_path / "sizes.c", tmp_path / "sizes"
    src.write_text('#include <stdio.h>\n#include "lightplane_hip_hash_grid.h"\nint main(void){printf("%zu\\n", '
                   'sizeof(LpHashGridArgs)); return 0;}\n')
    subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert int(subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE).stdout.split()[0]) == L.lp_abi_sizeof(38)


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

    def bad(code, starts, **fields):
        a = _args()
        for k, v in fields.items():
            if isinstance(v, tuple):
                getattr(a, k)[v[0]] = v[1]
            else:
                setattr(a, k, v)
        assert _call(name, a) == code and _err().startswith(starts), (fields, _err())

    bad(-1, "offset[1]", offset=(1, 120))           # overlaps the level before
    bad(-1, "size[0]", size=(0, 125))               # a dense level is (N + 1)^3 rounded up to 8
    bad(-1, "size[2]", size=(2, 255))               # a hashed size is a power of two
    bad(-1, "entries", entries=895)                 # the levels end at 896
    bad(-1, "n_levels", n_levels=33)
    bad(-2, "features_per_level 3", features_per_level=3)
    a = _args(n_levels=16, features_per_level=8, log2_table_size=8, base_resolution=4, finest_resolution=64)
    a.n_levels, a.resolution[16], a.size[16], a.hashed[16], a.offset[16], a.entries = 17, 64, 256, 1, a.entries, a.entries + 256
    assert _call(name, a) == -2 and "136 channels > 128" in _err(), _err()   # (a 17th level by hand: hash_grid_layout stops at 128)
    assert _call(name, _args(n_rays=1 << 24, n_pts=128)) == -2 and "2^31" in _err(), _err()
    assert _call(name, _args(n_rays=-1)) == -1
    for n_rays, n_pts in ((0, 70), (3, 0)):   # an empty batch passes every check and launches nothing
        assert _call(name, _args(n_rays=n_rays, n_pts=n_pts)) == 0, _err()


def test_layout_against_hand_computed_tables():
    lay = lp.hash_grid_layout(4, 2, 8, 4, 32)   # T = 256: S^3 = 125 fits, 729 and up do not
    assert lay == (4, 2, 8, (4, 8, 16, 32), (0, 128, 384, 640), (128, 256, 256, 256), (False, True, True, True), 896, 8)
    assert lp.hash_grid_layout(2, 1, 8, 5, 5)[3:8] == ((5, 5), (0, 216), (216, 216), (False, False), 432)   # S^3 = 216 <= 256: dense
    lay = lp.hash_grid_layout()                  # the default: 16 levels from 16 to 2048 in a 2^19 table
    assert lay.resolutions[:5] == (16, 22, 30, 42, 58) and lay.resolutions[-1] == 2048 and lay.channels == 32
    assert lay.hashed == (False,) * 5 + (True,) * 11   # 59^3 = 205 379 fits 2^19, the next level's lattice does not
    assert lay.sizes[:2] == (4920, 12168) and lay.entries == sum(lay.sizes)
    assert lp.hash_grid_layout(1, 8, 3, 1, 1)[3:8] == ((1,), (0,), (8,), (False,), 8)
    for kw in (dict(n_levels=0), dict(n_levels=33), dict(features_per_level=3), dict(n_levels=32, features_per_level=8),
               dict(log2_table_size=2), dict(log2_table_size=25), dict(base_resolution=0), dict(base_resolution=64, finest_resolution=32),
               dict(finest_resolution=65537)):
        with pytest.raises(ValueError):
            lp.hash_grid_layout(**kw)


def test_python_surface():
    for name in hash_grid.__all__:
        assert name in lp.__all__ and getattr(lp, name) is getattr(hash_grid, name)
    lay = lp.hash_grid_layout(**HG.MIXED)
    table = lp.init_hash_grid(lay, 2, scale=0.5, generator=torch.Generator().manual_seed(1))
    assert table.shape == (2, 896, 2) and table.dtype == torch.float32 and 0.4 < float(table.abs().max()) <= 0.5
    pts, idx = torch.zeros(3, 5, 3), torch.zeros(3, dtype=torch.int64)
    for wrong in (table[:, :-8], table[..., :1], table[0], torch.zeros(2, 896, 4)):
        with pytest.raises(ValueError, match=r"table has to be a \[B, 896, 2\]"):
            lp.hash_grid_encode(pts, wrong, idx, lay)
    with pytest.raises(ValueError, match="layout"):
        lp.hash_grid_encode(pts, table, idx, tuple(lay))
    with pytest.raises(AssertionError, match="table has to be float32"):
        lp.hash_grid_encode(pts, table.double(), idx, lay)
    with pytest.raises(AssertionError, match="integer"):
        lp.hash_grid_encode(pts, table, idx.float(), lay)
    with pytest.raises(_lib.LightplaneHipError, match="GPU only"):   # there is no CPU path
        lp.hash_grid_encode(pts, table, idx, lay)


@pytest.mark.parametrize("name", HG.ALL)
def test_exclusion_caps_hold(name):
    c = HG.case(name)
    n, zeroed, left = c["zeroed"].numel(), int(c["zeroed"].sum()), int(c["left_out"].sum())
    print(f"{name}: {n} points, {zeroed} without a point gradient, {left} left out (cube face), {int((~c['inside']).sum())} masked")
    assert zeroed <= HG.MAX_ZEROED * n and left <= HG.MAX_LEFT_OUT * n
    assert c["mask"] or left == 0
    assert float(c["want"].abs().max()) > 0.1 and float(c["d_points"].abs().max()) > 0 and float(c["d_table"].abs().max()) > 0
    assert name != "masked" or 0 < int(c["inside"].sum()) < n

"""CPU tests of the host side of ``hash_grid_eval_mlp``: symbols, ABI struct and header, one refusal per class and entry point (before
anything touches a device), the wrapper's errors, and the exclusion caps of tests/hash_points_cases.py from its fp64 reference."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib, hash_grid
from tests import hash_points_cases as HP
from tests.synth import random_decoder

FAKE, STEP = 0x10000, 0x1000000  # 16-byte-aligned non-NULL "device pointers": no check dereferences them
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("lp_hash_points_forward", "lp_hash_points_backward")
POINTERS = ("table", "grad_table", "points", "grid_idx", "mlp_params", "encoding", "scaffold", "opacity_out", "color_out", "grad_opacity",
            "grad_color", "grad_mlp_params", "grad_encoding", "grad_points")
NEEDED = {EXPORTS[0]: ("table", "points", "grid_idx", "mlp_params", "encoding", "opacity_out"),
          EXPORTS[1]: ("table", "points", "grid_idx", "mlp_params", "encoding")}


def _decoder(lay, n_t=2, hidden=32):
    return random_decoder(torch.Generator().manual_seed(5), n_t, 2, 2, lay.channels, hidden, 3)


def _args(n_rays=3, n_pts=70, layout=None, dec=None):
    lay = lp.hash_grid_layout(**(layout or HP.MIXED))
    dec = dec or _decoder(lay)
    dims = [tuple(hash_grid.int_list_of(v)) for v in (dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color)]
    cfg = hash_grid._EvalCfg(hash_grid._Cfg(lay, False, False), *dims, 3, 1.0, False)
    a = hash_grid._eval_args(cfg, torch.zeros(1, 1, 3), torch.zeros(2, 1, 1), dec.mlp_params, torch.zeros(1, dims[2][0]), torch.zeros(1),
                             torch.zeros(2, 5, 4, 6), True)
    a.n_rays, a.n_pts = n_rays, n_pts
    for i, f in enumerate(POINTERS):
        setattr(a, f, FAKE + i * STEP)
    return a


_err = lambda: _lib.lib().lp_last_error().decode()  # noqa: E731
_call = lambda name, a: getattr(_lib.lib(), name)(ctypes.byref(a), None)  # noqa: E731


def test_symbols_struct_and_header(tmp_path):
    L = _lib.lib()
    text = open(os.path.join(ROOT, "include", "lightplane_hip_hash_points.h")).read()
    assert _lib.HASH_POINTS_EXPORTS == EXPORTS == tuple(re.findall(r"^int (lp_\w+)\(", text, re.M))
    assert all(hasattr(L, n) and n not in _lib.EXPORTS + _lib.HASH_GRID_EXPORTS for n in EXPORTS)
    assert L.lp_abi_sizeof(42) == ctypes.sizeof(_lib.LpHashPointsArgs)
    assert [L.lp_abi_sizeof(w) for w in (40, 41, 43)] == [-1, -1, -1] and L.lp_version() == 207
    from lightplane_amd.csrc import build as B
    assert any(h.endswith("lightplane_hip_hash_points.h") for h in B.PUBLIC_HEADERS) and "lp_hash_points.hip" in B.SOURCES
    cc = shutil.which("cc") or shutil.which("gcc")   # (a C compiler is needed: the header has to pass it as plain C)
    src, exe = tmp_path / "sizes.c", tmp_path / "sizes"
    src.write_text('#include <stdio.h>\n#include "lightplane_hip_hash_points.h"\nint main(void){printf("%zu\\n", '
                   'sizeof(LpHashPointsArgs)); return 0;}\n')
    subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert int(subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE).stdout.split()[0]) == L.lp_abi_sizeof(42)


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

    def bad(code, has, **fields):
        a = _args()
        for k, v in fields.items():
            if isinstance(v, tuple):
                getattr(a, k)[v[0]] = v[1]
            else:
                setattr(a, k, v)
        assert _call(name, a) == code and has in _err(), (fields, _err())

    bad(-1, "offset[1]", offset=(1, 120))                     # the layout rules are those of lp_hash_grid_*
    bad(-1, "size[2]", size=(2, 255))
    bad(-2, "features_per_level 3", features_per_level=3)
    bad(-1, "trunk MLP input width 8 != grid channels 6", n_levels=3)   # the trunk reads L * F features
    bad(-1, "encoding_dim 31", encoding_dim=31)
    bad(-1, "color_chn 0", color_chn=0)
    bad(-1, "mlp_params has 10", n_mlp_params=10)
    bad(-1, "scaffold_shape: batch 3", scaffold_shape=_lib.LpGrid(3, 5, 4, 6, 0, None))
    lay8 = lp.hash_grid_layout(**dict(HP.MIXED, n_levels=16, features_per_level=2))
    assert _call(name, _args(dec=_decoder(lay8, 0), layout=dict(HP.MIXED, n_levels=4))) == -1 and "opacity MLP input width 32 != 8" in _err()
    assert _call(name, _args(n_rays=1 << 24, n_pts=128)) == -2 and "2^31" in _err(), _err()
    assert _call(name, _args(n_rays=-1)) == -1
    if name == EXPORTS[1]:   # the backward keeps every layer's activations of a point: at most 1024 floats
        lay = lp.hash_grid_layout(**dict(HP.MIXED, n_levels=16, features_per_level=8))
        wide = random_decoder(torch.Generator().manual_seed(5), 4, 4, 2, lay.channels, 128, 3)
        assert _call(name, _args(dec=wide, layout=dict(HP.MIXED, n_levels=16, features_per_level=8))) == -2 and "exceeds 1024" in _err()
    for n_rays, n_pts in ((0, 70), (3, 0)):   # an empty batch passes every check and launches nothing
        assert _call(name, _args(n_rays=n_rays, n_pts=n_pts)) == 0, _err()


def test_python_surface():
    for name in hash_grid.__all__:
        assert name in lp.__all__ and getattr(lp, name) is getattr(hash_grid, name)
    lay = lp.hash_grid_layout(**HP.MIXED)
    table, dec = lp.init_hash_grid(lay, 2), _decoder(lay)
    pts, idx, enc = torch.zeros(3, 5, 3), torch.zeros(3, dtype=torch.int64), torch.zeros(3, 32)
    with pytest.raises(ValueError, match=r"table has to be a \[B, 896, 2\]"):
        lp.hash_grid_eval_mlp(pts, table[:, :-8], idx, lay, dec, enc, 1.0)
    narrow = lp.hash_grid_layout(**dict(HP.MIXED, n_levels=3))
    with pytest.raises(ValueError, match="the decoder reads 8 features, the layout has n_levels x features_per_level = 6"):
        lp.hash_grid_eval_mlp_opacity_only(pts, lp.init_hash_grid(narrow, 2), idx, narrow, dec, 1.0)
    with pytest.raises(AssertionError, match="table has to be float32"):
        lp.hash_grid_eval_mlp(pts, table.double(), idx, lay, dec, enc, 1.0)
    with pytest.raises(AssertionError, match=r"rays_encoding has to be a \[3, 32\]"):
        lp.hash_grid_eval_mlp(pts, table, idx, lay, dec, enc[:, :8], 1.0)
    with pytest.raises(_lib.LightplaneHipError, match="GPU only"):   # there is no CPU path
        lp.hash_grid_eval_mlp(pts, table, idx, lay, dec, enc, 1.0)


@pytest.mark.parametrize("name", HP.ALL)
def test_exclusion_caps_hold(name):
    c = HP.case(name)
    n, zeroed, left = c["zeroed"].numel(), int(c["zeroed"].sum()), int(c["left_out"].sum())
    print(f"{name}: {n} points, {zeroed} with a zero upstream gradient, {left} left out, {int((~c['inside']).sum())} masked, "
          f"{int((c['occ'] == 0).sum())} with occ = 0")
    assert zeroed <= HP.MAX_ZEROED * n and left <= HP.MAX_LEFT_OUT * n
    assert float(c["op"].abs().max()) > 0.1 and all(float(g.abs().max()) > 0 for g in c["grads"].values())
    assert name != "contract_mask_scaffold" or 0 < int((c["occ"] == 0).sum()) < n
    assert name != "masked_112x32" or 0 < int(c["inside"].sum()) < n

"""CPU tests of the host side of ``hash_grid_render_samples``: symbols, ABI struct and header, one refusal per class and entry point
(before anything touches a device), the wrapper's errors, and the case table of tests/hash_render_cases.py from its fp64 reference."""
import ctypes
import dataclasses
import os
import re
import shutil
import subprocess

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib, hash_grid
from tests import compositing_cases as CC
from tests import hash_render_cases as HC
from tests import render_samples_cases as RC
from tests.synth import random_decoder

FAKE, STEP = 0x10000, 0x1000000  # 16-byte-aligned non-NULL "device pointers": no check dereferences them
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("lp_hash_render_forward", "lp_hash_render_backward")
POINTERS = ("table", "grad_table", "mlp_params", "scaffold", "origins", "directions", "grid_idx", "encoding", "depths", "deltas", "ray_length",
            "neg_log_t", "feature", "weights", "chunk_nlt", "grad_ray_length", "grad_neg_log_t", "grad_feature", "grad_weights",
            "grad_mlp_params", "grad_encoding")
NEEDED = ("table", "mlp_params", "origins", "directions", "grid_idx", "encoding", "depths", "deltas")


def _decoder(lay, n_t=2, hidden=32):
    return random_decoder(torch.Generator().manual_seed(5), n_t, 2, 2, lay.channels, hidden, 3)


def _args(n_rays=3, n_samples=70, layout=None, dec=None):
    lay = lp.hash_grid_layout(**(layout or HC.MIXED))
    dec = dec or _decoder(lay)
    dims = [tuple(hash_grid.int_list_of(v)) for v in (dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color)]
    cfg = hash_grid._RenderCfg(hash_grid._Cfg(lay, False, False), *dims, 3, 1.0, True, True)
    z = torch.zeros(1, 1)
    a = hash_grid._render_args(cfg, z, z, z, z, z, torch.zeros(2, 5, 4, 6), torch.zeros(2, 1, 1), dec.mlp_params, torch.zeros(1, dims[2][0]), True)
    a.n_rays, a.n_samples = n_rays, n_samples
    for i, f in enumerate(POINTERS):
        setattr(a, f, FAKE + i * STEP)
    return a


_err = lambda: _lib.lib().lp_last_error().decode()  # noqa: E731
_call = lambda name, a: getattr(_lib.lib(), name)(ctypes.byref(a), None)  # noqa: E731


def test_symbols_struct_and_header(tmp_path):
    L = _lib.lib()
    text = open(os.path.join(ROOT, "include", "lightplane_hip_hash_render.h")).read()
    assert _lib.HASH_RENDER_EXPORTS == EXPORTS == tuple(re.findall(r"^int (lp_\w+)\(", text, re.M))
    assert all(hasattr(L, n) and n not in _lib.EXPORTS + _lib.HASH_GRID_EXPORTS + _lib.HASH_POINTS_EXPORTS for n in EXPORTS)
    assert L.lp_abi_sizeof(46) == ctypes.sizeof(_lib.LpHashRenderArgs)
    assert [L.lp_abi_sizeof(w) for w in (44, 45, 47)] == [-1, -1, -1] and L.lp_version() == 207
    hr = _lib.build_info()["points"]["hash_render"]   # (no new top-level key: the text's keys are pinned)
    assert "one wavefront per ray" in hr["forward"] and "run-merged" in hr["backward"]
    from lightplane_amd.csrc import build as B
    assert any(h.endswith("lightplane_hip_hash_render.h") for h in B.PUBLIC_HEADERS) and "lp_hash_render.hip" in B.SOURCES
    cc = shutil.which("cc") or shutil.which("gcc")   # (a C compiler is needed: the header has to pass it as plain C)
    src, exe = tmp_path / "sizes.c", tmp_path / "sizes"
    src.write_text('#include <stdio.h>\n#include "lightplane_hip_hash_render.h"\nint main(void){printf("%zu\\n", '
                   'sizeof(LpHashRenderArgs)); return 0;}\n')
    subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert int(subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE).stdout.split()[0]) == L.lp_abi_sizeof(46)


@pytest.mark.parametrize("name", EXPORTS)
def test_refusals(name):
    """each refusal class once per entry point; none reaches a device"""
    assert getattr(_lib.lib(), name)(None, None) == -3 and "args is NULL" in _err()
    for f in NEEDED + (("chunk_nlt",) if name == EXPORTS[1] else ()):
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
    bad(-2, "features_per_level 3", features_per_level=3)
    bad(-1, "trunk MLP input width 8 != grid channels 6", n_levels=3)   # the trunk reads L * F features
    bad(-1, "encoding_dim 31", encoding_dim=31)
    bad(-1, "scaffold_shape: batch 3", scaffold_shape=_lib.LpGrid(3, 5, 4, 6, 0, None))
    bad(-1, "n_samples 0 < 1", n_samples=0)
    assert _call(name, _args(n_rays=1 << 24, n_samples=128)) == -2 and "2^31" in _err(), _err()
    a = _args()   # without the colour head (no feature / no upstream for it) the encoding and the colour MLP are not looked at
    a.feature = a.grad_feature = a.encoding = None
    a.encoding_dim, a.color.n_layers, a.n_rays = 0, 0, 0
    assert _call(name, a) == 0, _err()
    if name == EXPORTS[1]:   # the backward keeps every layer's activations of a sample: at most 1024 floats
        wide_lay = dict(HC.MIXED, n_levels=16, features_per_level=8)
        wide = random_decoder(torch.Generator().manual_seed(5), 4, 4, 2, 128, 128, 3)
        assert _call(name, _args(dec=wide, layout=wide_lay)) == -2 and "exceeds 1024" in _err()
    assert _call(name, _args(n_rays=0)) == 0, _err()   # an empty batch passes every check and launches nothing


def test_python_surface():
    assert "hash_grid_render_samples" in lp.__all__ and lp.hash_grid_render_samples is hash_grid.hash_grid_render_samples
    c = HC.inputs("mixed_222x32")
    depths, deltas = HC.host_samples("mixed_222x32")
    call = lambda r=c["rays"], d=depths, dl=deltas, t=c["table"], lay=c["lay"], **kw: lp.hash_grid_render_samples(  # noqa: E731
        r, d, dl, t, lay, c["dec"], **kw)
    with pytest.raises(ValueError, match=r"table has to be a \[B, 896, 2\]"):
        call(t=c["table"][:, :-8])
    with pytest.raises(ValueError, match="the decoder reads 8 features, the layout has n_levels x features_per_level = 6"):
        narrow = lp.hash_grid_layout(**dict(HC.MIXED, n_levels=3))
        call(lay=narrow, t=lp.init_hash_grid(narrow, 2))
    with pytest.raises(AssertionError, match="rays.encoding"):
        call(r=dataclasses.replace(c["rays"], encoding=None))
    for kw in (dict(), dict(with_color=False, return_weights=True, r=dataclasses.replace(c["rays"], encoding=None))):
        with pytest.raises(_lib.LightplaneHipError, match="GPU only"):   # there is no CPU path
            call(**kw)
    for what in ("depths", "deltas", "origins", "directions"):
        r, kw = c["rays"], {}
        if what in ("depths", "deltas"):
            kw = {"d" if what == "depths" else "dl": (depths if what == "depths" else deltas).clone().requires_grad_(True)}
        else:
            r = dataclasses.replace(r, **{what: getattr(r, what).clone().requires_grad_(True)})
        with pytest.raises(NotImplementedError, match=rf"{what}.*\.detach\(\).*modular chain"):
            call(r=r, **kw)


@pytest.mark.parametrize("name", HC.ALL)
def test_zeroed_share_is_within_the_cap(name):
    c = HC.case(name, *HC.host_samples(name))
    n, zeroed = c["zeroed"].numel(), int(c["zeroed"].sum())
    print(f"{name}: {n} samples, {zeroed} zeroed, gain {c['gain']:.4g}, median -log T {float(c['out'][1].median()):.4g}, zero deltas "
          f"{int((c['deltas'] == 0).sum())}")
    assert c["depths"].shape == (c["R"], c["S"]) and zeroed <= HC.MAX_ZEROED * n
    if name == "opaque":
        assert abs(float(c["out"][1].median()) - 800.0) < 1e-6 and bool((torch.exp(-c["out"][1].float()) == 0).any())


def test_the_definition_is_the_chain_composed_in_fp64():
    """at the depths of ray_samples, deltas untouched: the field at the oracle's points, composited"""
    c = HC.inputs("mixed_222x32")
    r64 = dataclasses.replace(c["rays"], **{k: getattr(c["rays"], k).double() for k in ("origins", "directions", "near", "far")})
    points, depths, deltas = CC.placement(r64, c["S"], 0, RC.DISPARITY, torch.float64)
    leaves = dict(table=c["table"].double(), params=c["dec"].mlp_params.double(), enc=c["rays"].encoding.double())
    with torch.no_grad():
        op, col, _, _ = HC.field(c, points, leaves)
        want = CC.composite(1.7 * op, col, depths, deltas)
        op2, col2, _, _ = HC.field(c, HC.points_of(c, depths), leaves)
        got = CC.composite(1.7 * op2, col2, depths, deltas)
    for a, b in zip(got, want):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))

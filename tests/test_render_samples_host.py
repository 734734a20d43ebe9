"""CPU tests of the host side of ``render_samples``: the fp64 definition the GPU test compares with (tests/render_samples_cases.py) is
the oracle Renderer at uniform depths, the case table covers what it says, the three lp_render_samples_* symbols, their ABI struct and
the header of their own (include/lightplane_hip_render_samples.h), every argument check (before anything touches a device) and the
Python surface."""
import ctypes
import importlib
import inspect
import os
import re
import shutil
import subprocess

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib, grids
from oracle import lightplane_oracle as O
from tests import compositing_cases as CC
from tests import render_samples_cases as RC

RSM = importlib.import_module("lightplane_amd.render_samples")  # (the package attribute of that name is the function)
FAKE = 0x10000  # 16-byte-aligned non-NULL "device pointers": no check dereferences them, and every call below fails a check
STEP = 0x1000000  # (or has no rays to launch for)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lightplane_hip_render_samples.h")
EXPORTS = ("lp_render_samples_forward", "lp_render_samples_backward", "lp_render_samples_chunks")
POINTERS = ("mlp_params", "origins", "directions", "grid_idx", "encoding", "depths", "deltas", "scaffold", "ray_length", "neg_log_t",
            "feature", "weights", "chunk_nlt", "grad_ray_length", "grad_neg_log_t", "grad_feature", "grad_weights", "grad_grid",
            "grad_color_grid", "grad_mlp_params", "grad_encoding")
REQUIRED = ("origins", "directions", "grid_idx", "encoding", "depths", "deltas")


def _args(n_rays=3, n_samples=70, hidden=32):
    a = _lib.LpRenderSamplesArgs()
    a.grid = _lib.make_grid_list(None, [grids.GridDesc(1, 4, 4, 4, 0)], 16, 64)
    a.grid.data = FAKE + 50 * STEP
    dims = ([16, hidden, hidden], [hidden, hidden, 1], [hidden, hidden, 3])
    n = [sum(i * o + o for i, o in zip(d[:-1], d[1:])) for d in dims]
    a.trunk, a.opacity, a.color = _lib.make_mlp(dims[0], 0), _lib.make_mlp(dims[1], n[0]), _lib.make_mlp(dims[2], n[0] + n[1])
    a.n_mlp_params, a.color_chn, a.gain, a.encoding_dim = sum(n), 3, 1.0, hidden
    a.n_rays, a.n_samples = n_rays, n_samples
    for i, f in enumerate(POINTERS):
        if f not in ("scaffold", "grad_color_grid"):
            setattr(a, f, FAKE + i * STEP)
    return a


def _err():
    return _lib.lib().lp_last_error().decode()


def _call(name, a):
    return getattr(_lib.lib(), name)(ctypes.byref(a), None)


# ------------------------------------------------------------------------------------------------------------------------------
# the definition and the case table
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,S,S_inf", [("triplane_c16_222x32", 65, 0), ("voxel_c32_twogrid_022x32", 63, 3),
                                          ("triplane_c16_322x64_contract_mask_scaffold", 64, 3), ("voxel_c5_222x7", 2, 0)])
def test_the_definition_is_the_oracle_renderer_at_uniform_depths(name, S, S_inf):
    sc, rays = RC.scene(name), RC.rays_for(name, 9)
    r64 = lp.Rays(directions=rays.directions.double(), origins=rays.origins.double(), grid_idx=rays.grid_idx, near=rays.near.double(),
                  far=rays.far.double(), encoding=rays.encoding.double())
    _, depths, deltas = CC.placement(r64, S, S_inf, RC.DISPARITY, torch.float64)
    with torch.no_grad():
        got = RC.definition(sc, rays, depths, deltas, 1.7, sc["contract"])
        dec = sc["dec"]
        dec64 = lp.DecoderParams(dec.mlp_params.double(), dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
        want = O.lightplane_renderer_naive(
            r64, [g.double() for g in sc["grids"]], dec64, S, 1.7, mask_out_of_bounds_samples=sc["mask"], num_samples_inf=S_inf,
            contract_coords=sc["contract"], disparity_at_inf=RC.DISPARITY, scaffold=None if sc["scaffold"] is None else sc["scaffold"].double(),
            color_grid=None if sc["cgrids"] is None else [g.double() for g in sc["cgrids"]])
    for key, a, b in zip(("ray_length", "neg_log_t", "feature"), got, want):
        err = float((a - b[..., :3] if key == "feature" else a - b).abs().max())
        print(f"{name} S {S}+{S_inf} {key}: max |definition - oracle Renderer| = {err:.3e}")
        assert err <= 1e-12 * max(1.0, float(b.abs().max())), (name, key, err)
    assert torch.allclose(got[3].sum(-1), 1.0 - torch.exp(-got[1]), atol=1e-12)  # (the weights telescope to 1 - T)


def test_the_table_covers_what_it_says():
    cases = RC.CASES
    print(f"{len(cases)} cases:")
    for c in cases:
        print("  ", RC.case_id(c), "samples as", RC.split_samples(c[2], c[3]))
    assert len(set(cases)) == len(cases)
    assert {c[0] for c in cases} == set(RC.SHAPES) and {c[1] for c in cases} == set(RC.RS) and {c[2] for c in cases} == set(RC.SS)
    for name in RC.SHAPES:
        assert sum(c[0] == name for c in cases) >= 3, name
    for S in RC.SS:
        assert len({c[0] for c in cases if c[2] == S}) >= 3, S
    plain = [c for c in cases if not RC.scene(c[0])["jumps"]]
    assert {(c[3], c[4]) for c in plain} == {(d, o) for d in RC.DEPTHS for o in RC.OPACITIES}
    assert (1, 1) in {(c[1], c[2]) for c in cases} and (130, 200) in {(c[1], c[2]) for c in cases}
    # S on both sides of a chunk of 64 and over several chunks; the scene with jumps and the 128-wide decoder over more than one chunk
    assert any(RC.scene(c[0])["jumps"] and c[2] > 64 for c in cases) and ("triplane_c16_222x128", 130, 200, "resampled", "mixed") in cases
    for c in cases:
        a, b = RC.split_samples(c[2], c[3])
        assert a + b == c[2] and a >= 1 and (c[3] != "resampled" or (a >= 3 and b >= 1))
    assert sorted(n for n in RC.SHAPES if RC.scene(n)["jumps"]) == ["triplane_c16_322x64_contract_mask_scaffold"]
    w = RC.peaked_weights(9, 21)
    assert bool(((w > 0).sum(-1) == 1).all()) and len(set(w.argmax(-1).tolist())) > 1
    for S in (3, 21, 66):
        d = torch.rand(9, S).cumsum(-1)
        p, j = RC.peaked_depths(d), RC.peak_index(9, S)
        assert int(j.min()) >= 1 and int(j.max()) <= S - 2 and bool((p[:, 1:] >= p[:, :-1]).all())
        r = torch.arange(9)
        assert torch.equal(p[r, j - 1], p[r, j]) and torch.equal(p[r, j + 1], p[r, j]) and torch.equal(RC.peaked_weights(9, S).argmax(-1), j)


def test_gains_put_the_batch_in_its_regime():
    name, R, S = "triplane_c16_222x32", 9, 65
    sc, rays = RC.scene(name), RC.rays_for(name, R)
    _, depths, deltas = CC.placement(rays, S, 0, RC.DISPARITY, torch.float32)
    for regime, want in (("transparent", 0.05), ("opaque", 800.0)):
        g = RC.gain_for(sc, rays, depths, deltas, False, regime)
        with torch.no_grad():
            out = RC.definition(sc, rays, depths.double(), deltas.double(), g, False)
        nlt = out[1]
        print(f"{regime}: gain {g:.4g}, median -log T {float(nlt.median()):.4g}")
        assert abs(float(nlt.median()) - want) <= 1e-9 * want
        if regime == "opaque":  # exp(-x) is 0 in fp32 from x = 104 on: half the rays pass that before the ray ends (1 - T is 1 there)
            assert float(nlt.median()) > 4 * 104 and float((out[3].sum(-1) == 1.0).float().mean()) >= 0.5
    assert RC.gain_for(sc, rays, depths, deltas, False, "mixed") == 1.7
    assert RC.gain_for(sc, rays, depths, torch.zeros_like(deltas), False, "opaque") == 1.7


# ------------------------------------------------------------------------------------------------------------------------------
# symbols, struct, header
# ------------------------------------------------------------------------------------------------------------------------------

def test_symbols_struct_and_tables():
    L = _lib.lib()
    assert _lib.RENDER_SAMPLES_EXPORTS == EXPORTS
    for name in EXPORTS:
        assert hasattr(L, name), f"{name} not exported by liblightplane_hip.so"
        for table in (_lib.EXPORTS, _lib.SAMPLES_EXPORTS, _lib.IMPORTANCE_EXPORTS, _lib.LOSSES_EXPORTS):
            assert name not in table  # (the tables of the other headers stay as they are)
    assert L.lp_abi_sizeof(30) == ctypes.sizeof(_lib.LpRenderSamplesArgs)
    for which in (27, 28, 29, 31, 32):
        assert L.lp_abi_sizeof(which) == -1, which
    assert L.lp_version() == 207  # additive: no version change
    info = _lib.build_info()
    rs = info["points"]["render_samples"]  # (no new top-level key: the text's keys are pinned)
    assert "one wavefront per ray" in rs["forward"] and "no atomics" in rs["backward"]
    from lightplane_amd.csrc import build as B
    assert info["src_hash"] == B.source_hash()
    assert any(h.endswith("lightplane_hip_render_samples.h") for h in B.PUBLIC_HEADERS) and "lp_render_samples.hip" in B.SOURCES
    assert any(h.endswith("lightplane_hip_render_samples.h") for h in B.HEADERS)
    for s, want in ((-1, 0), (0, 0), (1, 1), (64, 1), (65, 2), (200, 4), (2 ** 31 - 1, 2 ** 25)):
        assert L.lp_render_samples_chunks(s) == want == RSM.chunks(s), s


def test_header_declares_the_bound_symbols_and_is_plain_c(tmp_path):
    text = open(HEADER).read()
    assert tuple(re.findall(r"^int (lp_\w+)\(", text, re.M)) == EXPORTS
    assert '#include "lightplane_hip.h"' in text
    for other in ("lightplane_hip.h", "lightplane_hip_samples.h", "lightplane_hip_importance.h", "lightplane_hip_losses.h"):
        declared = re.findall(r"^int (lp_\w+)\(", open(os.path.join(ROOT, "include", other)).read(), re.M)
        assert not set(EXPORTS) & set(declared), other
    assert '#include "../../include/lightplane_hip_render_samples.h"' in open(os.path.join(ROOT, "lightplane_amd", "csrc", "lp_host.h")).read()
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None, "a C compiler (cc or gcc) is needed: the header has to pass it as plain C"
    subprocess.run([cc, "-x", "c", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", HEADER], check=True)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "lightplane_hip_render_samples.h"\nint main(void){printf("%zu\\n", '
                   'sizeof(LpRenderSamplesArgs)); return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    size = int(subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE).stdout.split()[0])
    assert size == ctypes.sizeof(_lib.LpRenderSamplesArgs) == _lib.lib().lp_abi_sizeof(30)


# ------------------------------------------------------------------------------------------------------------------------------
# refusals (none reaches a device)
# ------------------------------------------------------------------------------------------------------------------------------

def test_null_arguments_are_refused():
    L = _lib.lib()
    for name in EXPORTS[:2]:
        assert getattr(L, name)(None, None) == -3 and "args is NULL" in _err(), name
        for f in REQUIRED + (("chunk_nlt",) if name.endswith("backward") else ()):
            a = _args()
            setattr(a, f, None)
            assert _call(name, a) == -3 and _err().startswith(f"{f} is NULL"), (name, f, _err())
        a = _args()
        a.mlp_params = None
        assert _call(name, a) == -3 and "mlp_params is NULL" in _err(), _err()
        a = _args()
        a.grid.data = None
        assert _call(name, a) == -3 and "grid.data is NULL" in _err(), _err()
    # an empty batch passes every check and launches nothing; so does a backward without any upstream gradient ... on no rays
    a = _args(n_rays=0)
    for f in POINTERS:
        if f != "mlp_params":
            setattr(a, f, None)
    for name in EXPORTS[:2]:
        assert _call(name, a) == 0, (name, _err())


def test_under_aligned_pointers_are_refused():
    for off in (4, 8, 12):
        for name in EXPORTS[:2]:
            for n_rays in (3, 0):  # (whatever n_rays is)
                for f in POINTERS:
                    a = _args(n_rays=n_rays)
                    setattr(a, f, FAKE + 40 * STEP + off)
                    assert _call(name, a) == -1 and _err().startswith(f"{f} = ") and "16-byte aligned" in _err(), (name, f, off, _err())
                a = _args(n_rays=n_rays)
                a.grad_grid_list[0] = FAKE + 40 * STEP + off
                assert _call(name, a) == -1 and _err().startswith("grad_grid_list[0] = "), _err()
                a = _args(n_rays=n_rays)
                a.grid.data = FAKE + 40 * STEP + off
                assert _call(name, a) == -1 and _err().startswith("grid.data = "), _err()


def test_malformed_shapes_are_refused():
    for name in EXPORTS[:2]:
        assert _call(name, _args(n_rays=-1)) == -1 and "n_rays -1" in _err(), _err()
        for s in (0, -3):
            assert _call(name, _args(n_samples=s)) == -1 and _err().startswith(f"n_samples {s} < 1"), _err()
        assert _call(name, _args(n_rays=1 << 24, n_samples=128)) == -2 and "2^31" in _err(), _err()   # R S = 2^31
        a = _args(n_rays=(1 << 24) - 1, n_samples=128)   # (below 2^31: the next failing check refuses)
        a.encoding_dim = 31
        assert _call(name, a) == -1 and "encoding_dim 31" in _err(), _err()
        a = _args()
        a.color_chn = 4
        assert _call(name, a) == -1 and "color_chn 4" in _err(), _err()
        a = _args()
        a.n_mlp_params -= 1
        assert _call(name, a) == -1 and "mlp_params has" in _err(), _err()
        a = _args()
        a.grid.n_grids = 0
        assert _call(name, a) == -1 and "empty grid-list" in _err(), _err()
        a = _args()
        a.scaffold, a.scaffold_shape = FAKE, _lib.LpGrid(2, 4, 4, 4, 0, None)
        assert _call(name, a) == -1 and "scaffold shape" in _err(), _err()
        a = _args()
        a.grad_grid, a.grad_grid_list[0] = None, None
        a.grid = _lib.make_grid_list(None, [grids.GridDesc(1, 1, 4, 4, 0), grids.GridDesc(1, 4, 1, 4, 16)], 16, 32)
        a.grid.data = FAKE
        a.grad_grid_list[1] = FAKE + STEP
        if name.endswith("backward"):
            assert _call(name, a) == -1 and "all or none" in _err(), _err()


def test_python_surface():
    assert "render_samples" in lp.__all__ and lp.render_samples is RSM.render_samples
    sig = inspect.signature(lp.render_samples)
    assert list(sig.parameters) == ["rays", "depths", "deltas", "grid", "decoder_params", "gain", "mask_out_of_bounds_samples",
                                    "contract_coords", "scaffold", "color_grid", "grid_sizes", "color_grid_sizes", "return_weights"]
    for name, default in (("gain", 1.0), ("mask_out_of_bounds_samples", False), ("contract_coords", False), ("scaffold", None),
                          ("color_grid", None), ("grid_sizes", None), ("color_grid_sizes", None), ("return_weights", False)):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[name].default == default, name
    msig = inspect.signature(lp.LightplaneRenderer.render_samples)
    assert list(msig.parameters)[:4] == ["self", "rays", "feature_grid", "samples"]
    assert msig.parameters["return_weights"].kind is inspect.Parameter.KEYWORD_ONLY and msig.parameters["return_weights"].default is False
    name = "triplane_c16_222x32"
    sc, rays = RC.scene(name), RC.rays_for(name, 9)
    _, depths, deltas = CC.placement(rays, 5, 0, RC.DISPARITY, torch.float32)
    call = lambda r=rays, d=depths, dl=deltas, **kw: lp.render_samples(r, d, dl, sc["grids"], sc["dec"], **kw)  # noqa: E731
    with pytest.raises(_lib.LightplaneHipError, match="GPU only"):   # there is no CPU path: tensors that pass every check need a GPU
        call()
    with pytest.raises(AssertionError, match="Rays object"):
        call(r=None)
    with pytest.raises(AssertionError, match="depths"):
        call(d=depths[0])
    with pytest.raises(AssertionError, match="deltas"):
        call(dl=deltas[:, :4])
    with pytest.raises(AssertionError, match="rays.origins"):
        call(d=depths[:5], dl=deltas[:5])
    with pytest.raises(AssertionError, match="depths has to be float32"):
        call(d=depths.double())
    with pytest.raises(AssertionError, match="deltas has to be float32"):
        call(dl=deltas.double())
    huge = torch.zeros(1, 1).expand(1 << 16, 1 << 15)   # R S = 2^31: shapes only, nothing is allocated
    with pytest.raises(AssertionError, match=r"depths.*2\^31"):
        lp.render_samples(rays, huge, huge, sc["grids"], sc["dec"])
    no_enc = lp.Rays(directions=rays.directions, origins=rays.origins, grid_idx=rays.grid_idx, near=rays.near, far=rays.far)
    with pytest.raises(AssertionError, match="rays.encoding"):
        call(r=no_enc)
    for what in ("depths", "deltas", "origins", "directions"):
        kw = dict(directions=rays.directions, origins=rays.origins, grid_idx=rays.grid_idx, near=rays.near, far=rays.far, encoding=rays.encoding)
        d, dl = depths, deltas
        if what == "depths":
            d = depths.clone().requires_grad_(True)
        elif what == "deltas":
            dl = deltas.clone().requires_grad_(True)
        else:
            kw[what] = kw[what].clone().requires_grad_(True)
        with pytest.raises(NotImplementedError, match=rf"{what}.*\.detach\(\).*modular chain"):
            call(r=lp.Rays(**kw), d=d, dl=dl)
        with torch.no_grad(), pytest.raises(_lib.LightplaneHipError, match="GPU only"):   # (grad mode off: nothing to refuse)
            call(r=lp.Rays(**kw), d=d, dl=dl)

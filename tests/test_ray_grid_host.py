"""CPU tests of the host side of ``splat_along_rays`` / ``gather_along_rays``: the three lp_ray_grid_* symbols, their ABI struct and the
header of their own (include/lightplane_hip_ray_grid.h), every argument check (before anything touches a device), the Python surface,
and the inputs of the fp64 oracle the GPU test compares with (tests/ray_grid_cases.py): its exclusion caps and what its table covers."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib, grids, ray_grid
from tests import point_grid_cases as PC
from tests import ray_grid_cases as RG

FAKE = 0x10000  # 16-byte-aligned non-NULL "device pointers": no check dereferences them, and every call below fails a check
STEP = 0x1000000  # (or has nothing to launch for)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lightplane_hip_ray_grid.h")
EXPORTS = ("lp_ray_grid_splat", "lp_ray_grid_gather", "lp_ray_grid_grad_samples")
POINTERS = ("origins", "directions", "grid_idx", "depths", "weights", "vectors", "out_features", "grad_weights", "grad_depths")
REQUIRED = ("origins", "directions", "grid_idx", "depths", "weights")
BUILD_INFO_KEYS = ["version", "src_hash", "test_hooks", "tuned_bwd", "loop_bwd_deep", "loop_bwd_shallow", "mlp_splatter_bwd",
                   "loop_fwd_stream", "grid_tv", "grid_resample", "scaffold", "points", "ray_clip", "point_grid", "mesh", "forward", "flags"]


def _args(n_rays=3, n_samples=70, channels=16):
    a = _lib.LpRayGridArgs()
    a.grid = _lib.make_grid_list(None, [grids.GridDesc(1, 4, 4, 4, 0)], channels, 64)
    a.grid.data = FAKE + 50 * STEP
    a.channels = channels
    a.n_rays, a.n_samples = n_rays, n_samples
    for i, f in enumerate(POINTERS):
        setattr(a, f, FAKE + i * STEP)
    return a


def _err():
    return _lib.lib().lp_last_error().decode()


def _call(name, a):
    return getattr(_lib.lib(), name)(ctypes.byref(a), None)


# ------------------------------------------------------------------------------------------------------------------------------
# symbols, struct, header
# ------------------------------------------------------------------------------------------------------------------------------

def test_symbols_struct_and_tables():
    L = _lib.lib()
    assert _lib.RAY_GRID_EXPORTS == EXPORTS
    for name in EXPORTS:
        assert hasattr(L, name), f"{name} not exported by liblightplane_hip.so"
        for table in (_lib.EXPORTS, _lib.SAMPLES_EXPORTS, _lib.IMPORTANCE_EXPORTS, _lib.LOSSES_EXPORTS, _lib.RENDER_SAMPLES_EXPORTS):
            assert name not in table  # (the tables of the other headers stay as they are)
    assert L.lp_abi_sizeof(34) == ctypes.sizeof(_lib.LpRayGridArgs)
    for which in (28, 31, 32, 33, 35, 99):
        assert L.lp_abi_sizeof(which) == -1, which
    assert L.lp_version() == 207  # additive: no version change
    info = _lib.build_info()
    assert list(info) == BUILD_INFO_KEYS  # (no new key)
    from lightplane_amd.csrc import build as B
    assert info["src_hash"] == B.source_hash()
    assert any(h.endswith("lightplane_hip_ray_grid.h") for h in B.PUBLIC_HEADERS) and "lp_ray_grid.hip" in B.SOURCES
    assert any(h.endswith("lightplane_hip_ray_grid.h") for h in B.HEADERS)


def test_header_declares_the_bound_symbols_and_is_plain_c(tmp_path):
    text = open(HEADER).read()
    assert tuple(re.findall(r"^int (lp_\w+)\(", text, re.M)) == EXPORTS
    assert '#include "lightplane_hip.h"' in text
    for other in ("lightplane_hip.h", "lightplane_hip_samples.h", "lightplane_hip_importance.h", "lightplane_hip_losses.h",
                  "lightplane_hip_render_samples.h"):
        declared = re.findall(r"^int (lp_\w+)\(", open(os.path.join(ROOT, "include", other)).read(), re.M)
        assert not set(EXPORTS) & set(declared), other
    assert '#include "../../include/lightplane_hip_ray_grid.h"' in open(os.path.join(ROOT, "lightplane_amd", "csrc", "lp_host.h")).read()
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None, "a C compiler (cc or gcc) is needed: the header has to pass it as plain C"
    subprocess.run([cc, "-x", "c", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", HEADER], check=True)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "lightplane_hip_ray_grid.h"\nint main(void){printf("%zu\\n", '
                   'sizeof(LpRayGridArgs)); return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    size = int(subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE).stdout.split()[0])
    assert size == ctypes.sizeof(_lib.LpRayGridArgs) == _lib.lib().lp_abi_sizeof(34)


# ------------------------------------------------------------------------------------------------------------------------------
# refusals (none reaches a device)
# ------------------------------------------------------------------------------------------------------------------------------

def test_null_arguments_are_refused():
    L = _lib.lib()
    for name in EXPORTS:
        assert getattr(L, name)(None, None) == -3 and "args is NULL" in _err(), name
        for f in REQUIRED:
            a = _args()
            setattr(a, f, None)
            assert _call(name, a) == -3 and _err().startswith(f"{f} is NULL"), (name, f, _err())
        a = _args()
        a.grid.data = None
        assert _call(name, a) == -3 and "grid.data is NULL" in _err(), _err()
    for name in ("lp_ray_grid_splat", "lp_ray_grid_grad_samples"):  # the missing vector
        a = _args()
        a.vectors = None
        assert _call(name, a) == -3 and _err().startswith("vectors is NULL"), (name, _err())
    a = _args()  # the missing result
    a.out_features = None
    assert _call("lp_ray_grid_gather", a) == -3 and _err().startswith("out_features is NULL"), _err()
    a = _args()
    a.grad_weights = a.grad_depths = None
    assert _call("lp_ray_grid_grad_samples", a) == -3 and _err().startswith("grad_weights and grad_depths are both NULL"), _err()
    # an empty batch passes every check and launches nothing
    for n_rays, n_samples in ((0, 70), (3, 0), (0, 0)):
        for name in EXPORTS:
            assert _call(name, _args(n_rays=n_rays, n_samples=n_samples)) == 0, (name, _err())


def test_under_aligned_pointers_are_refused():
    for off in (4, 8, 12):
        for name in EXPORTS:
            for n_rays in (3, 0):  # (whatever n_rays is)
                for f in POINTERS:
                    a = _args(n_rays=n_rays)
                    setattr(a, f, FAKE + 40 * STEP + off)
                    assert _call(name, a) == -1 and _err().startswith(f"{f} = ") and "16-byte aligned" in _err(), (name, f, off, _err())
                a = _args(n_rays=n_rays)
                a.row_weight[0] = FAKE + 40 * STEP + off
                assert _call(name, a) == -1 and _err().startswith("row_weight[0] = "), _err()
                a = _args(n_rays=n_rays)
                a.grid.data = FAKE + 40 * STEP + off
                assert _call(name, a) == -1 and _err().startswith("grid.data = "), _err()


def test_malformed_shapes_are_refused():
    for name in EXPORTS:
        assert _call(name, _args(n_rays=-1)) == -1 and _err().startswith("n_rays -1 < 0"), _err()
        assert _call(name, _args(n_samples=-3)) == -1 and _err().startswith("n_samples -3 < 0"), _err()
        assert _call(name, _args(n_rays=1 << 24, n_samples=128)) == -2 and "2^31" in _err(), _err()   # R S = 2^31
        a = _args(n_rays=(1 << 24) - 1, n_samples=128)   # (below 2^31: the next failing check refuses)
        a.channels = 15
        assert _call(name, a) == -1 and _err().startswith("channels 15") and "grid channels 16" in _err(), _err()
        for c in (0, 129):
            assert _call(name, _args(channels=c)) == -2 and f"{c} channels outside [1, 128]" in _err(), _err()
        a = _args()
        a.grid.n_grids = 0
        assert _call(name, a) == -1 and "empty grid-list" in _err(), _err()
    a = _args()
    a.grid = _lib.make_grid_list(None, [grids.GridDesc(1, 1, 4, 4, 0), grids.GridDesc(1, 4, 1, 4, 16)], 16, 32)
    a.grid.data = FAKE
    a.row_weight[1] = FAKE + STEP
    assert _call("lp_ray_grid_splat", a) == -1 and "all or none" in _err(), _err()


# ------------------------------------------------------------------------------------------------------------------------------
# the Python surface
# ------------------------------------------------------------------------------------------------------------------------------

def _rays(c, **over):
    kw = dict(directions=c["directions"], origins=c["origins"], grid_idx=c["gidx"], near=torch.zeros(len(c["gidx"])),
              far=torch.ones(len(c["gidx"])))
    kw.update(over)
    return lp.Rays(**kw)


def test_python_surface():
    assert "splat_along_rays" in lp.__all__ and "gather_along_rays" in lp.__all__
    assert lp.splat_along_rays is ray_grid.splat_along_rays and lp.gather_along_rays is ray_grid.gather_along_rays
    assert ray_grid.__all__ == ["splat_along_rays", "gather_along_rays"]
    sig = inspect.signature(lp.splat_along_rays)
    assert list(sig.parameters) == ["rays", "depths", "weights", "features", "output_grid_size", "mask_out_of_bounds_samples",
                                    "contract_coords", "normalize", "return_list"]
    for name, default in (("mask_out_of_bounds_samples", False), ("contract_coords", False), ("normalize", False), ("return_list", True)):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[name].default is default, name
    sig = inspect.signature(lp.gather_along_rays)
    assert list(sig.parameters) == ["rays", "depths", "weights", "grid", "mask_out_of_bounds_samples", "contract_coords", "grid_sizes"]
    for name, default in (("mask_out_of_bounds_samples", False), ("contract_coords", False), ("grid_sizes", None)):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[name].default is default, name

    c = RG.case("triplane_c16")
    rays, t, w, f = _rays(c), c["depths"], c["weights"], c["feat"]
    splat = lambda r=rays, d=t, ww=w, ff=f, **kw: lp.splat_along_rays(r, d, ww, ff, c["sizes"], **kw)  # noqa: E731
    gather = lambda r=rays, d=t, ww=w, **kw: lp.gather_along_rays(r, d, ww, c["grids"], **kw)  # noqa: E731
    for call in (splat, gather):
        with pytest.raises(_lib.LightplaneHipError, match="GPU only"):   # there is no CPU path: tensors that pass every check need a GPU
            call()
        with pytest.raises(AssertionError, match="Rays object"):
            call(r=None)
        with pytest.raises(AssertionError, match="depths"):
            call(d=t[0])
        with pytest.raises(AssertionError, match="weights"):
            call(ww=w[:, :4])
        with pytest.raises(AssertionError, match="rays.origins"):
            call(d=t[:5], ww=w[:5])
        with pytest.raises(AssertionError, match="depths has to be float32"):
            call(d=t.double())
        with pytest.raises(AssertionError, match="weights has to be float32"):
            call(ww=w.double())
        with pytest.raises(AssertionError, match="integer"):
            call(r=_rays(c, grid_idx=c["gidx"].float()))
        huge = torch.zeros(1, 1).expand(1 << 16, 1 << 15)   # R S = 2^31: shapes only, nothing is allocated
        with pytest.raises(AssertionError, match=r"depths.*2\^31"):
            call(d=huge, ww=huge)
        # origins and directions get no gradient
        for what in ("origins", "directions"):
            r = _rays(c, **{what: c[what].clone().requires_grad_(True)})
            with pytest.raises(NotImplementedError, match=rf"rays\.{what}.*\.detach\(\).*o \+ t·d → splat_points / sample_grid_at_points"):
                call(r=r)
            with torch.no_grad(), pytest.raises(_lib.LightplaneHipError, match="GPU only"):   # (grad mode off: nothing to refuse)
                call(r=r)
    with pytest.raises(AssertionError, match=r"features has to be a \[7, 16\]"):
        splat(ff=f[:, :15])
    with pytest.raises(NotImplementedError, match="grid should be either tensor or list"):
        lp.gather_along_rays(rays, t, w, tuple(c["grids"]))
    # no gradient through the normalisation
    for what in ("weights", "depths"):
        kw = {"ww" if what == "weights" else "d": c[what].clone().requires_grad_(True)}
        with pytest.raises(NotImplementedError, match=rf"normalize=True\) has no gradient with respect to {what}.*normalize=False"):
            splat(normalize=True, **kw)
        with pytest.raises(_lib.LightplaneHipError, match="GPU only"):   # the raw splat differentiates them
            splat(**kw)
        with torch.no_grad(), pytest.raises(_lib.LightplaneHipError, match="GPU only"):
            splat(normalize=True, **kw)
    with pytest.raises(_lib.LightplaneHipError, match="GPU only"):   # features may always require one
        splat(ff=f.clone().requires_grad_(True), normalize=True)


# ------------------------------------------------------------------------------------------------------------------------------
# the cases of the GPU test
# ------------------------------------------------------------------------------------------------------------------------------

def test_exclusion_caps_hold():
    assert (RG.TOL, RG.CELL_EPS, RG.FACE_EPS, RG.MAX_LEFT_OUT, RG.MAX_ZEROED) == (PC.TOL, PC.CELL_EPS, PC.FACE_EPS, 0.02, 0.05)
    for name in RG.CASES:
        c = RG.case(name)
        n = c["depths"].numel()
        left, zeroed = int(c["left_out"].sum()), int(c["zeroed"].sum())
        print(f"{name}: {n} samples, {left} left out (cube face), {zeroed} without a depth gradient {c['counts']}, "
              f"{int(c['inside'].sum())} inside the cube")
        assert left <= RG.MAX_LEFT_OUT * n, name
        assert zeroed <= RG.MAX_ZEROED * n, name
        if not c["mask"]:
            assert left == 0, name
        if c["mask"] and c["normalize"]:
            assert left == 0, name  # (the splatted weights count every sample)
        assert torch.equal(c["w_kept"] == 0, (c["weights"] == 0) | c["left_out"])
        assert torch.equal(c["w_live"] == 0, (c["weights"] == 0) | c["zeroed"])


def test_the_table_covers_what_it_says():
    cases = {n: RG.case(n) for n in RG.CASES}
    shape = lambda n: tuple(cases[n]["depths"].shape)  # noqa: E731
    chans = lambda n: cases[n]["sizes"][0][4]  # noqa: E731
    assert shape("triplane_c16") == (7, 37) and chans("triplane_c16") == 16 and len(set(cases["triplane_c16"]["gidx"].tolist())) == 2
    c = cases["voxel_c32_flat"]
    assert shape("voxel_c32_flat")[1] == 70 and c["form"] == "flat" and c["gidx"].dtype == torch.int32 and chans("voxel_c32_flat") == 32
    assert all(cases[n]["gidx"].dtype == torch.int64 for n in cases if n != "voxel_c32_flat")
    assert chans("voxel_c5_mask") == 5 and cases["voxel_c5_mask"]["mask"]
    c = cases["triplane_c20_contract_mask"]
    assert chans("triplane_c20_contract_mask") == 20 and c["mask"] and c["contract"]
    assert 0 < int(c["inside"].sum()) and float(c["q64"].abs().max()) > 0.5  # (the contraction's outer branch is reached)
    assert chans("voxel_c128") == 128 and shape("voxel_c128")[1] == 3
    kinds = {sum(int(v > 1) for v in s[1:4]) for s in cases["mixed_list_c16"]["sizes"]}
    assert kinds == {2, 3} and len(cases["mixed_list_c16"]["sizes"]) == 4
    assert shape("one_sample") == (1, 1)
    # the mask removes something and keeps something (behind the contraction every point is inside)
    inside = cases["voxel_c5_mask"]["inside"]
    assert 0 < int(inside.sum()) < inside.numel()
    assert bool(cases["triplane_c20_contract_mask"]["inside"].all())

    def cells(n):  # the base cell of every sample of the case's (voxel) grid, [R, S, 3]
        c = cases[n]
        _, D, H, W, _ = c["sizes"][0]
        t = RG._unnorm(c["q64"], torch.tensor([W, H, D], dtype=torch.float64))
        return torch.floor(t).long()

    def runs(n):  # lengths of the runs of consecutive samples that share a base cell, chunks of 64 ignored
        out = []
        for row in cells(n):
            change = (row[1:] != row[:-1]).any(-1)
            edges = [0] + (torch.nonzero(change)[:, 0] + 1).tolist() + [len(row)]
            out += [b - a for a, b in zip(edges[:-1], edges[1:])]
        return out

    assert shape("one_cell") == (1, 70) and runs("one_cell") == [70]            # one run across the chunk boundary
    assert torch.equal(cells("one_cell")[0, 0], torch.tensor([1, 1, 1]))
    assert shape("dense_ray")[1] == 130 and max(runs("dense_ray")) >= 8 and len(runs("dense_ray")) >= 20   # many long runs
    assert max(runs("sparse_ray")) == 1                                          # no run longer than one
    d = cases["unsorted"]["depths"]
    assert bool((d[:, 1:] < d[:, :-1]).any(dim=1).all()) and bool((d[:, 1:] > d[:, :-1]).any(dim=1).all())
    for n in cases:
        if n != "unsorted":
            dd = cases[n]["depths"]
            assert bool((dd[:, 1:] >= dd[:, :-1]).all()), n
    w = cases["signed_weights"]["weights"]
    assert int((w == 0).sum()) > 0 and int((w < 0).sum()) > 0 and int((w > 0).sum()) > 0 and not cases["signed_weights"]["normalize"]
    assert all(cases[n]["normalize"] and float(cases[n]["weights"].min()) > 0 for n in cases if n != "signed_weights")


def test_the_oracle_is_the_bilinear_form_of_the_point_ops():
    """T(G, W, F; P) = B(G, P, U) with U[r, s] = W[r, s] F[r] (tests/point_grid_cases.py), and the normalised splat with weights 1 divides
    by the splat of ones"""
    for name in ("triplane_c16", "triplane_c20_contract_mask"):
        c = RG.case(name)
        g64 = [g.double() for g in c["grids"]]
        o, d, t, w, f = (c[k].double() for k in ("origins", "directions", "depths", "w_kept", "feat"))
        pts = t[..., None] * d[:, None, :] + o[:, None, :]
        u = w[..., None] * f[:, None, :]
        want = PC.bilinear_form(g64, pts, c["gidx"], u, c["mask"], c["contract"])
        got = RG.form_t(g64, o, d, c["gidx"], t, w, f, c["mask"], c["contract"])
        assert abs(float(got - want)) <= 1e-12 * abs(float(want)), name
        assert abs(float(sum((g * s).sum() for g, s in zip(g64, c["splat_raw"])) - want)) <= 1e-10 * abs(float(want)), name
        assert abs(float((c["gather"] * f).sum() - want)) <= 1e-10 * abs(float(want)), name

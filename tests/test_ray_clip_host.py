"""CPU tests of the ray clip's host side: the lp_rays_clip symbol and its ABI struct, every argument check of the C entry point (each
returns its code and message before anything touches a device), the Python wrapper's input checks, LightplaneRenderer.clip_rays under
contract_coords, and the condition on the test inputs of tests/test_gpu_ray_clip.py (tests/ray_clip_cases.py): at most 2 % of a case's
rays are ambiguous."""
import ctypes

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib, ray_clip
from tests import ray_clip_cases as RC

FAKE = 0x10000  # a 16-byte-aligned non-NULL "device pointer": no check dereferences it, and every call below fails a check or has no rays
OUT = 0x40000000


def _args(n_rays=8, scaffold=True, shape=(2, 5, 6, 7), pad=0.5):
    a = _lib.LpRayClipArgs()
    a.rays.n_rays = n_rays
    a.rays.directions, a.rays.origins, a.rays.grid_idx = FAKE, FAKE + 0x1000, FAKE + 0x2000
    a.rays.near_t, a.rays.far_t = FAKE + 0x3000, FAKE + 0x4000
    if scaffold:
        a.scaffold = FAKE + 0x100000
        a.scaffold_shape = _lib.LpGrid(*shape, 0, None)
    a.pad = pad
    return a


def _err():
    return _lib.lib().lp_last_error().decode()


def _clip(a, near=OUT, far=OUT + 0x1000, hit=OUT + 0x2001):  # (hit_out is bytes: any address)
    return _lib.lib().lp_rays_clip(ctypes.byref(a) if a is not None else None, near, far, hit, None)


def test_symbol_struct_and_build_info():
    L = _lib.lib()
    assert hasattr(L, "lp_rays_clip") and "lp_rays_clip" in _lib.EXPORTS
    assert L.lp_version() == 207
    assert L.lp_abi_sizeof(12) == ctypes.sizeof(_lib.LpRayClipArgs)
    assert L.lp_abi_sizeof(9) == -1 and L.lp_abi_sizeof(11) == -1 and L.lp_abi_sizeof(13) == -1 and L.lp_abi_sizeof(99) == -1
    info = _lib.build_info()
    assert "ray_clip" in info and "no atomics" in info["ray_clip"]["walk"] and "integer-bounded" in info["ray_clip"]["walk"]
    assert "scaffold" in info and "points" in info  # (its neighbours are still there)
    assert "clip_rays_to_scaffold" in lp.__all__ and lp.clip_rays_to_scaffold is ray_clip.clip_rays_to_scaffold
    assert hasattr(lp.LightplaneRenderer, "clip_rays")


def test_null_arguments_are_refused():
    assert _clip(None) == -3 and "args is NULL" in _err()
    for kw in ({"near": None}, {"far": None}, {"hit": None}):
        assert _clip(_args(), **kw) == -3 and "near_out / far_out / hit_out" in _err(), kw
    for field in ("directions", "origins", "grid_idx", "near_t", "far_t"):
        a = _args()
        setattr(a.rays, field, None)
        assert _clip(a) == -3 and "directions/origins/grid_idx/near/far" in _err(), field


def test_under_aligned_pointers_are_refused():
    for off in (4, 8, 2):
        for field in ("directions", "origins", "grid_idx", "near_t", "far_t"):
            a = _args()
            setattr(a.rays, field, FAKE + 0x8000 + off)
            assert _clip(a) == -1 and f"rays.{field}" in _err() and "16-byte aligned" in _err(), (field, off)
        a = _args()
        a.scaffold = FAKE + 0x100000 + off
        assert _clip(a) == -1 and "scaffold" in _err() and "16-byte aligned" in _err()
        assert _clip(_args(), near=OUT + off) == -1 and "near_out" in _err() and "16-byte aligned" in _err()
        assert _clip(_args(), far=OUT + 0x1000 + off) == -1 and "far_out" in _err() and "16-byte aligned" in _err()
    # the alignment rule holds whatever n_rays is; hit_out is bytes and carries none
    a = _args(n_rays=0)
    a.rays.near_t = FAKE + 4
    assert _clip(a) == -1 and "rays.near_t" in _err()
    assert _clip(_args(n_rays=0), hit=OUT + 0x2003) == 0


def test_bad_values_are_refused():
    assert _clip(_args(n_rays=-1)) == -1 and "n_rays -1 < 0" in _err()
    for bad in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert _clip(_args(pad=bad)) == -1 and "pad" in _err() and ">= 0 and finite" in _err(), bad
    for i, field in enumerate(("B", "D", "H", "W")):
        for bad in (0, -3):
            a = _args()
            setattr(a.scaffold_shape, field, bad)
            assert _clip(a) == -1 and "extent < 1" in _err(), (field, bad)
    # without a scaffold the shape is not looked at
    a = _args(n_rays=0, scaffold=False)
    a.scaffold_shape = _lib.LpGrid(0, 0, 0, 0, 0, None)
    assert _clip(a) == 0


def test_no_rays_succeed_without_a_launch():
    assert _clip(_args(n_rays=0)) == 0
    a = _args(n_rays=0, scaffold=False)
    a.rays.directions = a.rays.origins = a.rays.grid_idx = a.rays.near_t = a.rays.far_t = None  # (no rays: nothing to point at)
    assert _clip(a) == 0
    assert _clip(_args(n_rays=0), near=None) == -3  # ... but the results are asked for all the same


def _rays(n=5, **kw):
    f = dict(directions=torch.ones(n, 3), origins=torch.zeros(n, 3), grid_idx=torch.zeros(n, dtype=torch.int32), near=torch.zeros(n),
             far=torch.ones(n), encoding=None)
    f.update(kw)
    return lp.Rays(**f)


def test_wrapper_rejects_bad_arguments():
    sc = torch.ones(1, 2, 3, 4)
    with pytest.raises(AssertionError, match="Rays object"):
        lp.clip_rays_to_scaffold((torch.zeros(3, 3),), sc)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(AssertionError, match="pad has to be"):
            lp.clip_rays_to_scaffold(_rays(), sc, pad=bad)
    with pytest.raises(AssertionError, match="float32"):
        lp.clip_rays_to_scaffold(_rays(near=torch.zeros(5, dtype=torch.float64)), sc)
    with pytest.raises(AssertionError, match="float32"):
        lp.clip_rays_to_scaffold(_rays(), sc.double())
    with pytest.raises(AssertionError, match=r"\[B, D, H, W\]"):
        lp.clip_rays_to_scaffold(_rays(), sc[0])
    with pytest.raises(AssertionError, match="contiguous"):
        lp.clip_rays_to_scaffold(_rays(), torch.ones(1, 2, 4, 3).transpose(2, 3))
    with pytest.raises(AssertionError, match="contiguous"):
        lp.clip_rays_to_scaffold(_rays(directions=torch.ones(3, 5).t()), sc)
    # a tensor on another device than the rays is refused by _lib.check_tensors ("meta" stands in for a second device here)
    with pytest.raises(AssertionError, match="scaffold is on meta"):
        lp.clip_rays_to_scaffold(_rays(), sc.to("meta"))
    mixed = _rays()
    mixed.near = torch.zeros(5, device="meta")
    with pytest.raises(AssertionError, match="rays.near is on meta"):
        lp.clip_rays_to_scaffold(mixed, sc)
    # there is no CPU path: CPU tensors pass check_tensors (they share a device) and every other check, then need a GPU
    with pytest.raises(_lib.LightplaneHipError, match="GPU only"):
        lp.clip_rays_to_scaffold(_rays(), sc)
    with pytest.raises(_lib.LightplaneHipError, match="GPU only"):
        lp.clip_rays_to_scaffold(_rays())


def test_module_clip_rays_raises_under_contract_coords():
    kw = dict(num_samples=8, color_chn=3, grid_chn=8, mlp_hidden_chn=16)
    with pytest.raises(NotImplementedError, match="contract_coords"):
        lp.LightplaneRenderer(contract_coords=True, **kw).clip_rays(_rays(), torch.ones(1, 2, 3, 4))
    with pytest.raises(_lib.LightplaneHipError, match="GPU only"):  # (a straight-ray module passes the call on)
        lp.LightplaneRenderer(**kw).clip_rays(_rays(), torch.ones(1, 2, 3, 4))


@pytest.mark.parametrize("name", RC.CASE_NAMES)
def test_cases_are_unambiguous(name):
    """the cap on ambiguous rays is a condition on the inputs: from the oracle alone"""
    c = RC.case(name)
    assert len(c["kind"]) == RC.R == 257
    n = int(c["oracle"]["ambiguous"].sum())
    print(f"{name}: {n} of {RC.R} rays ambiguous, {int(c['oracle']['hit'].sum())} hit, {int(RC.tight_mask(c).sum())} in the tightness set")
    assert n <= RC.AMBIGUOUS_CAP * RC.R
    # the mix the cases promise
    assert not set(RC.GLIDER_NAMES) & set(RC.CASE_NAMES)  # (the face gliders are a family of their own: no cap, no oracle)
    kinds = set(c["kind"])
    assert {"generic", "miss_box", "near_inside", "far_before", "far_inside_object", "origin_in_occupied", "origin_in_box", "far_lt_near",
            "zero_1", "zero_2", "zero_3", "ill_conditioned", "non_finite", "grid_idx_out_of_range"} <= kinds
    assert c["kind"].count("ill_conditioned") == 8 and c["kind"].count("non_finite") == 4 and c["kind"].count("grid_idx_out_of_range") == 2
    d = c["d"]
    ill = torch.tensor([k == "ill_conditioned" for k in c["kind"]])
    small = d[ill].abs().min(dim=1).values
    assert bool(((small > 0) & (small < 1e-3 * d[ill].abs().max(dim=1).values)).all())
    for nz in (1, 2, 3):
        sel = torch.tensor([k == f"zero_{nz}" for k in c["kind"]])
        assert bool(((d[sel] == 0).sum(dim=1) >= nz).all())
    if name not in ("one_cell_empty", "zeros_8"):
        assert 0 < int(c["oracle"]["hit"].sum()) < RC.R

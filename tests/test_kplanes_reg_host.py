"""CPU tests of the K-Planes regularisers' host side: the lp_kplanes_reg_* symbols and the capability string, the workspace query,
every refusal of the C ABI (each returns its code and message before anything touches a device) and the wrappers' input checks."""
import ctypes

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib, regularizers

FAKE = 0x10000  # a 16-byte-aligned non-NULL "device pointer": no check dereferences it, and every call below fails a check
DYN = lp.kplanes_layout((5, 9), (4, 4), 8)
ENTRIES = ("lp_kplanes_reg_forward", "lp_kplanes_reg_backward", "lp_kplanes_reg_fused")


def _args(layout=DYN, batch=2, p=2):
    a = regularizers._reg_args(layout, batch)
    a.p = p
    a.planes, a.grad_planes, a.terms = FAKE, FAKE + 0x100, FAKE + 0x200
    return a


def _call(entry, a, ws=FAKE + 0x300, ws_bytes=None):
    L = _lib.lib()
    if entry == "lp_kplanes_reg_backward":
        return L.lp_kplanes_reg_backward(ctypes.byref(a), None)
    if ws_bytes is None:
        ws_bytes = L.lp_kplanes_reg_workspace_bytes(ctypes.byref(a))
    return getattr(L, entry)(ctypes.byref(a), ws, ws_bytes, None)


def _err():
    return _lib.lib().lp_last_error().decode()


def test_symbols_struct_and_capability_string():
    L = _lib.lib()
    for name in _lib.KPLANES_REG_EXPORTS:
        assert hasattr(L, name), f"{name} not exported by liblightplane_hip.so"
    assert set(ENTRIES) < set(_lib.KPLANES_REG_EXPORTS) and L.lp_abi_sizeof(62) == ctypes.sizeof(_lib.LpKPlanesRegArgs)
    assert [L.lp_abi_sizeof(w) for w in (60, 61, 63)] == [-1, -1, -1]
    info = _lib.build_info()["points"]["kplanes_reg"]   # (no new top-level key: the text's keys are pinned)
    assert info["terms"] == ["space_tv", "time_smoothness", "time_l1"] and info["p"] == [1, 2] and "no atomics" in info["reduction"]
    for name in ("kplanes_regularizers", "add_kplanes_reg_grad_", "kplanes_reg_workspace_bytes"):
        assert name in lp.__all__ and getattr(lp, name) is getattr(regularizers, name)
    from lightplane_amd.csrc import build as B
    assert any(h.endswith("lightplane_hip_kplanes_reg.h") for h in B.PUBLIC_HEADERS) and "lp_kplanes_reg.hip" in B.SOURCES


def test_workspace_bytes_positive_and_monotone_in_the_tile_count():
    last = 0
    for n in (2, 3, 16, 17, 32, 33, 64, 100, 129, 512):   # more strips of u and more chunks of i_v never need less
        b = lp.kplanes_reg_workspace_bytes(lp.kplanes_layout((n,), (n,), 32))
        assert b > 0 and b % 24 == 0 and b >= last, (n, b, last)
        last = b
    one = lp.kplanes_reg_workspace_bytes(DYN, 1)
    assert lp.kplanes_reg_workspace_bytes(DYN, 3) == 3 * one     # one double[3] per workgroup, the same workgroups per scene
    assert lp.kplanes_reg_workspace_bytes(lp.kplanes_layout((5, 9), None, 8)) < one   # the static layout has half the planes
    assert lp.kplanes_reg_workspace_bytes(lp.kplanes_layout((64, 128, 256, 512), 150, 32)) <= 1 << 20   # of a 189 MB field


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_c_abi_refuses(entry):
    L = _lib.lib()
    terms, grad = entry != ENTRIES[1], entry != ENTRIES[0]
    if entry == ENTRIES[1]:
        assert L.lp_kplanes_reg_backward(None, None) == -3 and "args is NULL" in _err()
    else:
        assert getattr(L, entry)(None, FAKE, 1 << 20, None) == -3 and "args is NULL" in _err()
    for field, used in (("planes", True), ("terms", terms), ("grad_planes", grad)):
        a = _args()
        setattr(a, field, None)
        if used:   # (every call of this file has to be refused: the pointers are fakes)
            assert _call(entry, a) == -3 and field + " is NULL" in _err()
        a = _args()
        setattr(a, field, FAKE + 4)
        assert _call(entry, a) == -1 and _err().startswith(field + " = ") and "16-byte aligned" in _err()
    for p in (0, 3, -1):
        assert _call(entry, _args(p=p)) == -1 and "p = " in _err()
    if terms:
        a = _args()
        need = L.lp_kplanes_reg_workspace_bytes(ctypes.byref(a))
        assert _call(entry, a, ws_bytes=need - 1) == -1 and "workspace of" in _err() and str(need) in _err()
        assert _call(entry, a, ws=None) == -3 and "workspace is NULL" in _err()
    if grad:
        a = _args()
        a.grad_planes = a.planes
        assert _call(entry, a) == -1 and "aliases" in _err()
    # a malformed layout table: offsets that do not match the sizes, too few rows, channels outside the set, a resolution below 2
    for field, index, value, code, word in (("offset", (0, 1), DYN.offsets[0][1] - 1, -1, "offset[0][1]"), ("rows", None, DYN.rows - 1, -1, "rows"),
                                            ("channels", None, 12, -2, "channels"), ("temporal", (1,), 1, -1, "temporal[1]"),
                                            ("batch", None, 0, -1, "batch"), ("n_planes", None, 4, -1, "n_planes")):
        a = _args()
        if index is None:
            setattr(a, field, value)
        elif len(index) == 1:
            getattr(a, field)[index[0]] = value
        else:
            getattr(a, field)[index[0]][index[1]] = value
        assert _call(entry, a, ws_bytes=1 << 20) == code and word in _err(), field
        assert L.lp_kplanes_reg_workspace_bytes(ctypes.byref(a)) == 0 and word in _err(), field   # (the query answers 0, with the message)
    assert L.lp_kplanes_reg_workspace_bytes(None) == 0 and "NULL" in _err()


def test_wrappers_refuse_bad_inputs():
    planes = torch.ones(2, DYN.rows, DYN.channels)
    grad = torch.zeros_like(planes)
    with pytest.raises(ValueError, match="KPlanesLayout"):
        lp.kplanes_regularizers(planes, (5, 9))
    for bad in (planes[:, 1:], planes[0], planes[..., :4], torch.ones(0, DYN.rows, DYN.channels), "planes"):
        with pytest.raises(ValueError, match="planes has to be"):
            lp.kplanes_regularizers(bad, DYN)
        with pytest.raises(ValueError, match="planes has to be"):
            lp.add_kplanes_reg_grad_(bad, grad, DYN)
    for p in (0, 3):
        with pytest.raises(AssertionError, match="p has to be"):
            lp.kplanes_regularizers(planes, DYN, p=p)
        with pytest.raises(AssertionError, match="p has to be"):
            lp.add_kplanes_reg_grad_(planes, grad, DYN, p=p)
    with pytest.raises(AssertionError, match="weights has 2 entries"):
        lp.add_kplanes_reg_grad_(planes, grad, DYN, weights=(1.0, 2.0))
    with pytest.raises(AssertionError, match="shaped like planes"):
        lp.add_kplanes_reg_grad_(planes, grad[:1], DYN)
    with pytest.raises(AssertionError, match="contiguous"):
        lp.add_kplanes_reg_grad_(planes, torch.zeros(2, DYN.rows, 2 * DYN.channels)[..., ::2], DYN)
    with pytest.raises(AssertionError, match="alias"):
        lp.add_kplanes_reg_grad_(planes, planes, DYN)
    with pytest.raises(AssertionError, match="float32"):
        lp.kplanes_regularizers(planes.double(), DYN)
    # there is no CPU path: tensors that pass every check still need a GPU
    with pytest.raises(_lib.LightplaneHipError, match="GPU only"):
        lp.kplanes_regularizers(planes, DYN)
    with pytest.raises(_lib.LightplaneHipError, match="GPU only"):
        lp.add_kplanes_reg_grad_(planes, grad, DYN)

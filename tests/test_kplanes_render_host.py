"""CPU tests of the host side of ``kplanes_render_samples``: the case table of tests/kplanes_render_cases.py from its fp64 reference
(every case inside its cap), the new ABI's struct and refusals (before anything touches a device) and the wrapper's errors."""
import ctypes
import dataclasses

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib, kplanes
from tests import kplanes_render_cases as KC
from tests.synth import random_decoder

FAKE, STEP = 0x10000, 0x1000000  # 16-byte-aligned non-NULL "device pointers": no check dereferences them
EXPORTS = ("lp_kplanes_render_forward", "lp_kplanes_render_backward")
POINTERS = ("planes", "grad_planes", "times", "mlp_params", "scaffold", "origins", "directions", "grid_idx", "encoding", "depths", "deltas",
            "ray_length", "neg_log_t", "feature", "weights", "chunk_nlt", "grad_ray_length", "grad_neg_log_t", "grad_feature",
            "grad_weights", "grad_mlp_params", "grad_encoding")
NEEDED = ("planes", "mlp_params", "origins", "directions", "grid_idx", "times", "encoding", "depths", "deltas")


def _args(n_rays=3, n_samples=70, dec=None):
    lay = lp.kplanes_layout(**KC.DYN)
    dec = dec or random_decoder(torch.Generator().manual_seed(5), 2, 2, 2, lay.out_channels, 32, 3)
    dims = [tuple(kplanes.int_list_of(v)) for v in (dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color)]
    cfg = kplanes._RenderCfg(kplanes._Cfg(lay, False, False), *dims, 3, 1.0, True, True)
    z = torch.zeros(1, 1)
    a = kplanes._render_args(cfg, z, z, z, torch.zeros(1), z, z, torch.zeros(2, 5, 4, 6), torch.zeros(2, 1, 1), dec.mlp_params,
                             torch.zeros(1, dims[2][0]), True)
    a.n_rays, a.n_samples = n_rays, n_samples
    for i, f in enumerate(POINTERS):
        setattr(a, f, FAKE + i * STEP)
    return a


_err = lambda: _lib.lib().lp_last_error().decode()  # noqa: E731
_call = lambda name, a: getattr(_lib.lib(), name)(ctypes.byref(a), None)  # noqa: E731


@pytest.mark.parametrize("name", KC.ALL)
def test_zeroed_share_is_within_the_cap(name):
    c = KC.case(name, *KC.host_samples(name))
    n, zeroed = c["zeroed"].numel(), int(c["zeroed"].sum())
    print(f"{name}: {n} samples, {zeroed} zeroed, gain {c['gain']:.4g}, median -log T {float(c['out'][1].median()):.4g}, untouched rows "
          f"{int(c['untouched'].sum())} of {c['untouched'].numel()}")
    assert c["depths"].shape == (c["R"], c["S"]) and zeroed <= KC.MAX_ZEROED * n
    assert not bool(c["zeroed"].all(-1).any()) or c["S"] == 1, "a whole ray is zeroed: a per-ray timestamp near a vertex"
    assert all(float(g.abs().max()) > 0 for g in c["grads"].values())
    if name == "opaque":
        assert abs(float(c["out"][1].median()) - 800.0) < 1e-6 and bool((torch.exp(-c["out"][1].float()) == 0).any())


@pytest.mark.parametrize("name", EXPORTS)
def test_abi_refusals(name):
    """each refusal class once per entry point; none reaches a device"""
    L = _lib.lib()
    assert _lib.KPLANES_RENDER_EXPORTS == EXPORTS and L.lp_abi_sizeof(58) == ctypes.sizeof(_lib.LpKPlanesRenderArgs)
    assert [L.lp_abi_sizeof(w) for w in (56, 57, 59)] == [-1, -1, -1]
    info = _lib.build_info()["points"]["kplanes_render"]   # (no new top-level key: the text's keys are pinned)
    assert "one wavefront per ray" in info["forward"] and "run-merged" in info["backward"]
    assert getattr(L, name)(None, None) == -3 and "args is NULL" in _err()
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
            setattr(a, k, v)
        assert _call(name, a) == code and has in _err(), (fields, _err())

    a = _args()
    a.offset[1][0] = 3   # a broken layout: the rules are those of lp_kplanes_*
    assert _call(name, a) == -1 and "offset[1][0]" in _err(), _err()
    bad(-2, "channels 12", channels=12)
    bad(-1, "trunk MLP input width 16 != grid channels 8", n_scales=1)   # the trunk reads n_scales * C features
    bad(-1, "encoding_dim 31", encoding_dim=31)
    bad(-1, "scaffold_shape: batch 3", scaffold_shape=_lib.LpGrid(3, 5, 4, 6, 0, None))
    bad(-1, "n_samples 0 < 1", n_samples=0)
    bad(-1, "time_per_point 2", time_per_sample=2)
    assert _call(name, _args(n_rays=1 << 24, n_samples=128)) == -2 and "2^31" in _err(), _err()
    a = _args()   # without the colour head (no feature / no upstream for it) the encoding and the colour MLP are not looked at
    a.feature = a.grad_feature = a.encoding = None
    a.encoding_dim, a.color.n_layers, a.n_rays = 0, 0, 0
    assert _call(name, a) == 0, _err()
    if name == EXPORTS[1]:   # the backward keeps every layer's activations of a sample: at most 1024 floats
        wide = random_decoder(torch.Generator().manual_seed(5), 4, 4, 2, 16, 128, 3)
        assert _call(name, _args(dec=wide)) == -2 and "exceeds 1024" in _err()
    assert _call(name, _args(n_rays=0)) == 0, _err()   # an empty batch passes every check and launches nothing


def test_python_surface():
    assert "kplanes_render_samples" in lp.__all__ and lp.kplanes_render_samples is kplanes.kplanes_render_samples
    c = KC.inputs("dynamic_222x32")
    given = dict(zip(("depths", "deltas"), KC.host_samples("dynamic_222x32")), times=c["times"])

    def call(rays=c["rays"], **kw):
        v = dict(given, **kw)
        return lp.kplanes_render_samples(rays, v["times"], v["depths"], v["deltas"], c["planes"], c["lay"], c["dec"])
    with pytest.raises(_lib.LightplaneHipError, match="GPU only"):   # there is no CPU path
        call()
    for what in ("depths", "deltas", "times", "origins", "directions"):
        with pytest.raises(NotImplementedError, match=rf"{what}.*\.detach\(\).*modular chain"):
            if what in given:
                call(**{what: given[what].clone().requires_grad_(True)})
            else:
                call(dataclasses.replace(c["rays"], **{what: getattr(c["rays"], what).clone().requires_grad_(True)}))

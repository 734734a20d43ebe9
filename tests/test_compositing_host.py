"""CPU tests of the host side of the modular march: the four lp_ray_samples_* / lp_composite_* symbols and their two ABI structs, the
header of their own (include/lightplane_hip_samples.h), every argument check (each returns its code and a message that begins with
the field, before anything touches a device), the Python signatures, and the fp64 closed form of the compositing gradient the
backward kernel implements against autograd of the fp64 definition (tests/compositing_cases.py)."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib, compositing
from tests import compositing_cases as CC

FAKE = 0x10000  # 16-byte-aligned non-NULL "device pointers": no check dereferences them, and every call below fails a check
STEP = 0x1000000  # (or has no rays to launch for)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lightplane_hip_samples.h")

RS_RAY_FIELDS = ("directions", "origins", "near_t", "far_t")
RS_FIELDS = ("points", "depths", "deltas", "grad_points", "grad_depths", "grad_deltas", "grad_origins", "grad_directions", "grad_near",
             "grad_far")
CP_FIELDS = ("opacity", "features", "depths", "deltas", "ray_length", "neg_log_t", "feature", "weights", "grad_ray_length",
             "grad_neg_log_t", "grad_feature", "grad_weights", "grad_opacity", "grad_features", "grad_depths", "grad_deltas")
BUILD_INFO_KEYS = ["version", "src_hash", "test_hooks", "tuned_bwd", "loop_bwd_deep", "loop_bwd_shallow", "mlp_splatter_bwd",
                   "loop_fwd_stream", "grid_tv", "grid_resample", "scaffold", "points", "ray_clip", "point_grid", "mesh", "forward", "flags"]


def _rs_args(n_rays=3, num_samples=5, num_samples_inf=2):
    a = _lib.LpRaySamplesArgs()
    a.rays.n_rays = n_rays
    for i, f in enumerate(RS_RAY_FIELDS + ("grid_idx", "encoding")):
        setattr(a.rays, f, FAKE + i * STEP)
    a.march = _lib.make_march(num_samples, num_samples_inf, False, False, 1e-5)
    for i, f in enumerate(RS_FIELDS):
        setattr(a, f, FAKE + (8 + i) * STEP)
    return a


def _cp_args(n_rays=3, n_samples=5, channels=4):
    a = _lib.LpCompositeArgs()
    a.n_rays, a.n_samples, a.channels = n_rays, n_samples, channels
    for i, f in enumerate(CP_FIELDS):
        setattr(a, f, FAKE + i * STEP)
    return a


def _err():
    return _lib.lib().lp_last_error().decode()


def _call(name, a):
    return getattr(_lib.lib(), name)(ctypes.byref(a), None)


def test_symbols_structs_and_tables():
    L = _lib.lib()
    assert _lib.SAMPLES_EXPORTS == ("lp_ray_samples_forward", "lp_ray_samples_backward", "lp_composite_forward", "lp_composite_backward")
    for name in _lib.SAMPLES_EXPORTS:
        assert hasattr(L, name), f"{name} not exported by liblightplane_hip.so"
        assert name not in _lib.EXPORTS  # (the table of lightplane_hip.h stays as it is)
    assert L.lp_abi_sizeof(18) == ctypes.sizeof(_lib.LpRaySamplesArgs) == 168
    assert L.lp_abi_sizeof(20) == ctypes.sizeof(_lib.LpCompositeArgs) == 144
    for which in (17, 19, 21, 99):
        assert L.lp_abi_sizeof(which) == -1, which
    assert L.lp_version() == 207  # additive: no version change
    assert list(_lib.build_info()) == BUILD_INFO_KEYS  # no new key


def test_header_declares_the_bound_symbols_and_is_plain_c(tmp_path):
    text = open(HEADER).read()
    assert tuple(re.findall(r"^int (lp_\w+)\(", text, re.M)) == _lib.SAMPLES_EXPORTS
    assert '#include "lightplane_hip.h"' in text
    # every buffer says whether it is written entirely or read; none is accumulated into
    for f in RS_FIELDS + CP_FIELDS:
        line = [ln for ln in text.splitlines() if re.search(rf"\b{f};", ln)]
        assert line and all("WRITTEN entirely" in ln or "read" in ln for ln in line), f
    main = open(os.path.join(ROOT, "include", "lightplane_hip.h")).read()
    assert not set(_lib.SAMPLES_EXPORTS) & set(re.findall(r"^int (lp_\w+)\(", main, re.M))
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None, "a C compiler (cc or gcc) is needed: the header has to pass it as plain C"
    subprocess.run([cc, "-x", "c", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", HEADER], check=True)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "lightplane_hip_samples.h"\nint main(void){printf("%zu %zu\\n", '
                   'sizeof(LpRaySamplesArgs), sizeof(LpCompositeArgs)); return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(v) for v in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE).stdout.split()]
    assert sizes == [ctypes.sizeof(_lib.LpRaySamplesArgs), ctypes.sizeof(_lib.LpCompositeArgs)]


def test_python_surface():
    for name in ("ray_samples", "composite_samples", "RaySamples"):
        assert name in lp.__all__ and getattr(lp, name) is getattr(compositing, name)
    assert lp.RaySamples._fields == ("points", "depths", "deltas")
    sig = inspect.signature(lp.ray_samples)
    assert list(sig.parameters) == ["rays", "num_samples", "num_samples_inf", "disparity_at_inf"]
    assert sig.parameters["num_samples_inf"].default == 0
    assert sig.parameters["disparity_at_inf"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["disparity_at_inf"].default == 1e-5
    sig = inspect.signature(lp.composite_samples)
    assert list(sig.parameters) == ["opacity", "features", "depths", "deltas", "return_weights"]
    assert sig.parameters["return_weights"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["return_weights"].default is False
    assert list(inspect.signature(lp.LightplaneRenderer.ray_samples).parameters) == ["self", "rays"]
    # there is no CPU path: tensors that pass every check still need a GPU
    rays = lp.Rays(directions=torch.ones(2, 3), origins=torch.zeros(2, 3), grid_idx=torch.zeros(2, dtype=torch.long),
                   near=torch.zeros(2), far=torch.ones(2))
    with pytest.raises(_lib.LightplaneHipError, match="GPU only"):
        lp.ray_samples(rays, 4)
    with pytest.raises(_lib.LightplaneHipError, match="GPU only"):
        lp.composite_samples(torch.zeros(2, 4), None, torch.zeros(2, 4), torch.zeros(2, 4))
    with pytest.raises(AssertionError, match="num_samples"):
        lp.ray_samples(rays, 0)
    with pytest.raises(AssertionError, match="depths"):
        lp.composite_samples(torch.zeros(2, 4), None, torch.zeros(2, 5), torch.zeros(2, 4))
    with pytest.raises(AssertionError, match="features"):
        lp.composite_samples(torch.zeros(2, 4), torch.zeros(2, 4), torch.zeros(2, 4), torch.zeros(2, 4))
    with pytest.raises(AssertionError, match="at most 128"):
        lp.composite_samples(torch.zeros(2, 4), torch.zeros(2, 4, 129), torch.zeros(2, 4), torch.zeros(2, 4))
    with pytest.raises(AssertionError, match="float32"):
        lp.composite_samples(torch.zeros(2, 4).double(), None, torch.zeros(2, 4), torch.zeros(2, 4))


def test_null_arguments_are_refused():
    L = _lib.lib()
    for name in _lib.SAMPLES_EXPORTS:
        assert getattr(L, name)(None, None) == -3 and _err().startswith("args is NULL"), name
    for name, extra in (("lp_ray_samples_forward", ("points", "depths", "deltas")), ("lp_ray_samples_backward", ())):
        for f in RS_RAY_FIELDS:
            a = _rs_args()
            setattr(a.rays, f, None)
            assert _call(name, a) == -3 and _err().startswith(f"rays.{f} is NULL"), (name, f, _err())
        for f in extra:
            a = _rs_args()
            setattr(a, f, None)
            assert _call(name, a) == -3 and _err().startswith(f"{f} is NULL"), (name, f, _err())
    for name, extra in (("lp_composite_forward", ("ray_length", "neg_log_t", "feature")), ("lp_composite_backward", ())):
        for f in ("opacity", "depths", "deltas", "features") + extra:
            a = _cp_args()
            setattr(a, f, None)
            assert _call(name, a) == -3 and _err().startswith(f"{f} is NULL"), (name, f, _err())
        a = _cp_args(channels=16)
        a.features = None
        assert _call(name, a) == -3 and _err().startswith("features is NULL with channels = 16"), _err()


def test_optional_pointers_may_be_null():
    """what a call does not need may be NULL: with no rays every check is passed and nothing is launched"""
    a = _rs_args(n_rays=0)
    a.rays.grid_idx = a.rays.encoding = None
    for f in RS_FIELDS:
        setattr(a, f, None)
    assert _call("lp_ray_samples_forward", a) == 0 and _call("lp_ray_samples_backward", a) == 0, _err()
    # grid_idx and encoding are not read: with rays, their absence is no error (the first failing check is another one)
    a = _rs_args()
    a.rays.grid_idx = a.rays.encoding = None
    a.points = None
    assert _call("lp_ray_samples_forward", a) == -3 and _err().startswith("points is NULL")
    a = _cp_args(n_rays=0, channels=0)
    for f in CP_FIELDS:
        setattr(a, f, None)
    assert _call("lp_composite_forward", a) == 0 and _call("lp_composite_backward", a) == 0, _err()
    a = _cp_args(channels=0)  # no features without channels; weights are optional
    a.features = a.feature = a.weights = None
    a.opacity = None
    assert _call("lp_composite_forward", a) == -3 and _err().startswith("opacity is NULL")


def test_zero_rays_over_fake_pointers_is_ok():
    for name in ("lp_ray_samples_forward", "lp_ray_samples_backward"):
        assert _call(name, _rs_args(n_rays=0)) == 0, (name, _err())
    for name in ("lp_composite_forward", "lp_composite_backward"):
        assert _call(name, _cp_args(n_rays=0)) == 0, (name, _err())
        assert _call(name, _cp_args(n_rays=0, channels=128)) == 0 and _call(name, _cp_args(n_rays=0, channels=0)) == 0, (name, _err())


def test_under_aligned_pointers_are_refused():
    for off in (4, 8, 12):
        for name in ("lp_ray_samples_forward", "lp_ray_samples_backward"):
            for n_rays in (3, 0):  # (whatever n_rays is)
                for f in RS_RAY_FIELDS + ("grid_idx", "encoding"):
                    a = _rs_args(n_rays=n_rays)
                    setattr(a.rays, f, FAKE + 40 * STEP + off)
                    assert _call(name, a) == -1 and _err().startswith(f"rays.{f} = ") and "16-byte aligned" in _err(), (name, f, off, _err())
                for f in RS_FIELDS:
                    a = _rs_args(n_rays=n_rays)
                    setattr(a, f, FAKE + 40 * STEP + off)
                    assert _call(name, a) == -1 and _err().startswith(f"{f} = ") and "16-byte aligned" in _err(), (name, f, off, _err())
        for name in ("lp_composite_forward", "lp_composite_backward"):
            for n_rays in (3, 0):
                for f in CP_FIELDS:
                    a = _cp_args(n_rays=n_rays)
                    setattr(a, f, FAKE + 40 * STEP + off)
                    assert _call(name, a) == -1 and _err().startswith(f"{f} = ") and "16-byte aligned" in _err(), (name, f, off, _err())


def test_malformed_shapes_are_refused():
    for name in ("lp_ray_samples_forward", "lp_ray_samples_backward"):
        assert _call(name, _rs_args(num_samples=0)) == -1 and _err().startswith("num_samples 0 < 1"), _err()
        assert _call(name, _rs_args(num_samples_inf=-1)) == -1 and _err().startswith("num_samples_inf -1 < 0"), _err()
        assert _call(name, _rs_args(n_rays=-1)) == -1 and _err().startswith("n_rays -1"), _err()
        assert _call(name, _rs_args(n_rays=1 << 20, num_samples=(1 << 11) - 3, num_samples_inf=3)) == -2 and _err().startswith("n_rays") and "2^31" in _err(), _err()
        a = _rs_args(n_rays=(1 << 20) - 1, num_samples=(1 << 11) - 3, num_samples_inf=3)  # (below 2^31: the next check refuses)
        a.rays.origins = None
        assert _call(name, a) == -3 and _err().startswith("rays.origins is NULL"), _err()
        assert _call(name, _rs_args(n_rays=1, num_samples=(1 << 31) - 1, num_samples_inf=1)) == -2 and "2^31" in _err(), _err()
    for name in ("lp_composite_forward", "lp_composite_backward"):
        assert _call(name, _cp_args(n_samples=0)) == -1 and _err().startswith("n_samples 0 < 1"), _err()
        assert _call(name, _cp_args(n_samples=-5)) == -1 and _err().startswith("n_samples -5 < 1"), _err()
        assert _call(name, _cp_args(n_rays=-1)) == -1 and _err().startswith("n_rays -1"), _err()
        assert _call(name, _cp_args(channels=-1)) == -2 and _err().startswith("channels -1 outside [0, 128]"), _err()
        assert _call(name, _cp_args(channels=129)) == -2 and _err().startswith("channels 129 outside [0, 128]"), _err()
        assert _call(name, _cp_args(n_rays=1 << 20, n_samples=1 << 11)) == -2 and _err().startswith("n_rays") and "2^31" in _err(), _err()
        assert _call(name, _cp_args(n_rays=1 << 31, n_samples=1)) == -2 and _err().startswith("n_rays"), _err()


def test_the_case_table_covers_the_agreed_shapes():
    assert CC.RS == (1, 63, 130) and CC.SS == (1, 2, 63, 64, 65, 131, 200) and CC.CS == (0, 1, 3, 4, 5, 32, 64, 67, 128)
    assert CC.TOL == 1e-4 and 28 <= len(CC.CASES) <= 36 and len(set(CC.CASES)) == len(CC.CASES)
    assert {c[0] for c in CC.CASES} == set(CC.RS) and {c[1] for c in CC.CASES} == set(CC.SS) and {c[2] for c in CC.CASES} == set(CC.CS)
    for S in CC.SS:  # every chunk count meets a vectorised, a scalar and (somewhere) a two-units-per-lane channel count
        cs = {c[2] for c in CC.CASES if c[1] == S}
        assert len(cs) >= 4, (S, cs)
    c = CC.inputs(130, 65, 3, "transparent")
    nlt = (c["opacity"] * c["deltas"]).sum(-1)
    assert 0.02 < float(nlt.mean()) < 0.1
    c = CC.inputs(130, 65, 3, "opaque")
    assert float((c["opacity"] * c["deltas"])[:, :3].sum(-1).min()) > 49.9
    c = CC.inputs(130, 65, 3, "mixed")
    assert float(c["opacity"][1::3].abs().max()) == 0.0 and float(c["opacity"][0, 32:].min()) == 1e6
    assert float(torch.exp(-(c["opacity"] * c["deltas"]).double().sum(-1))[0]) == 0.0  # T underflows, in fp64 as well


@pytest.mark.parametrize("S", [1, 65, 131, 200])
@pytest.mark.parametrize("regime", CC.REGIMES)
def test_closed_form_gradient_is_autograd_of_the_definition(S, regime):
    """the test of the test: the formula the backward kernel implements, in fp64, against autograd of the fp64 definition"""
    R, C = 7, 5
    c = CC.case(R, S, C, regime)
    d = {k: (v.double() if torch.is_tensor(v) else v) for k, v in c.items() if k not in ("grads", "grads_w", "out")}
    for key, g_w in (("grads", torch.zeros(R, S, dtype=torch.float64)), ("grads_w", d["g_w"])):
        got = CC.closed_form_gradients(d["opacity"], d["features"], d["depths"], d["deltas"], d["g_len"], d["g_nlt"], d["g_feat"], g_w)
        for name, a, b in zip(("opacity", "features", "depths", "deltas"), got, c[key]):
            scale = max(float(b.abs().max()), 1e-300)
            err = float((a - b).abs().max())
            print(f"S={S} {regime} {key} d {name}: max |err| {err:.3e} (max |ref| {scale:.3e})")
            assert err <= 1e-12 * max(scale, 1.0), (name, err)
    # and expm1 is the same weight as the plain difference, in fp64
    w = CC.composite(d["opacity"], d["features"], d["depths"], d["deltas"])[3]
    od = d["opacity"] * d["deltas"]
    T = torch.exp(-torch.cumsum(torch.nn.functional.pad(od, (1, 0)), -1))[:, :-1]
    assert float((w - T * (-torch.expm1(-od))).abs().max()) <= 1e-15


@pytest.mark.parametrize("name", list(CC.CHAIN_CASES))
def test_chain_inputs_are_admissible(name):
    """the seeds of the chain cases, from the fp64 oracle alone: the samples at a decoder kink stay under the cap, and what is left is
    a real test (non-zero, finite results and gradients)"""
    from tests import points_cases as PC
    c = CC.chain_case(name)
    n = c["kink"].numel()
    print(f"{name}: {n} samples, at a kink {int(c['kink'].sum())} {c['counts']}")
    assert n == CC.CHAIN_RAYS * (CC.CHAIN_S + CC.CHAIN_S_INF) and int(c["kink"].sum()) <= PC.MAX_LEFT_OUT * n, "change the seed"
    flat = [t for v in c["grads"].values() for t in (v if isinstance(v, list) else [v])]
    for t in list(c["out"]) + flat:
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0

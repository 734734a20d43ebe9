"""CPU tests of the host side of importance resampling: the two lp_importance_samples_* symbols and their ABI struct, the header of
their own (include/lightplane_hip_importance.h), every argument check (each returns its code and a message that begins with the field,
before anything touches a device), the Python surface, and the definition's own properties (tests/importance_cases.py): the accuracy
bar is one the fp32 restatement of the definition meets with a wide margin, the new depths ascend, the histogram of many samples is the
mass of the bins."""
import ctypes
import inspect
import math
import os
import re
import shutil
import subprocess

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib, importance
from tests import importance_cases as IC

FAKE = 0x10000  # 16-byte-aligned non-NULL "device pointers": no check dereferences them, and every call below fails a check
STEP = 0x1000000  # (or has no rays to launch for)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lightplane_hip_importance.h")
FIELDS = ("origins", "directions", "depths", "weights", "jitter", "out_points", "out_depths", "out_deltas", "grad_points", "grad_origins",
          "grad_directions")
REQUIRED = {"lp_importance_samples_forward": ("origins", "directions", "depths", "weights", "out_points", "out_depths", "out_deltas"),
            "lp_importance_samples_backward": ("directions", "out_depths", "grad_points")}
BUILD_INFO_KEYS = ["version", "src_hash", "test_hooks", "tuned_bwd", "loop_bwd_deep", "loop_bwd_shallow", "mlp_splatter_bwd",
                   "loop_fwd_stream", "grid_tv", "grid_resample", "scaffold", "points", "ray_clip", "point_grid", "mesh", "forward", "flags"]


def _args(n_rays=3, n_samples=5, n_importance=4, include_coarse=1, pad=1e-5):
    a = _lib.LpImportanceArgs()
    a.n_rays, a.n_samples, a.n_importance, a.include_coarse, a.pad = n_rays, n_samples, n_importance, include_coarse, pad
    for i, f in enumerate(FIELDS):
        setattr(a, f, FAKE + i * STEP)
    return a


def _err():
    return _lib.lib().lp_last_error().decode()


def _call(name, a):
    return getattr(_lib.lib(), name)(ctypes.byref(a), None)


def test_symbols_struct_and_tables():
    L = _lib.lib()
    assert _lib.IMPORTANCE_EXPORTS == ("lp_importance_samples_forward", "lp_importance_samples_backward")
    for name in _lib.IMPORTANCE_EXPORTS:
        assert hasattr(L, name), f"{name} not exported by liblightplane_hip.so"
        assert name not in _lib.EXPORTS and name not in _lib.SAMPLES_EXPORTS  # (the tables of the other two headers stay as they are)
    assert L.lp_abi_sizeof(22) == ctypes.sizeof(_lib.LpImportanceArgs) == 112
    for which in (21, 23, 99):
        assert L.lp_abi_sizeof(which) == -1, which
    assert L.lp_version() == 207  # additive: no version change
    assert list(_lib.build_info()) == BUILD_INFO_KEYS  # no new key
    from lightplane_amd.csrc import build as B
    assert _lib.build_info()["src_hash"] == B.source_hash()
    assert any(h.endswith("lightplane_hip_importance.h") for h in B.HEADERS) and "lp_importance.hip" in B.SOURCES


def test_header_declares_the_bound_symbols_and_is_plain_c(tmp_path):
    text = open(HEADER).read()
    assert tuple(re.findall(r"^int (lp_\w+)\(", text, re.M)) == _lib.IMPORTANCE_EXPORTS
    assert '#include "lightplane_hip.h"' in text
    assert int(re.search(r"#define LP_IMPORTANCE_MAX (\d+)", text).group(1)) == _lib.LP_IMPORTANCE_MAX == 2048
    # every buffer says whether it is written entirely or read; none is accumulated into
    for f in FIELDS:
        line = [ln for ln in text.splitlines() if re.search(rf"\b{f};", ln)]
        assert line and all("WRITTEN entirely" in ln or "read" in ln for ln in line), f
    for other in ("lightplane_hip.h", "lightplane_hip_samples.h"):
        declared = re.findall(r"^int (lp_\w+)\(", open(os.path.join(ROOT, "include", other)).read(), re.M)
        assert not set(_lib.IMPORTANCE_EXPORTS) & set(declared), other
    assert '#include "../../include/lightplane_hip_importance.h"' in open(os.path.join(ROOT, "lightplane_amd", "csrc", "lp_host.h")).read()
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None, "a C compiler (cc or gcc) is needed: the header has to pass it as plain C"
    subprocess.run([cc, "-x", "c", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", HEADER], check=True)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "lightplane_hip_importance.h"\nint main(void){printf("%zu\\n", '
                   'sizeof(LpImportanceArgs)); return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    size = int(subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE).stdout.split()[0])
    assert size == ctypes.sizeof(_lib.LpImportanceArgs) == _lib.lib().lp_abi_sizeof(22)


def test_python_surface():
    assert "importance_samples" in lp.__all__ and lp.importance_samples is importance.importance_samples
    sig = inspect.signature(lp.importance_samples)
    assert list(sig.parameters) == ["rays", "depths", "weights", "num_importance", "include_coarse", "pad", "jitter"]
    for name, default in (("include_coarse", True), ("pad", 1e-5), ("jitter", None)):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[name].default == default, name
    assert list(inspect.signature(lp.LightplaneRenderer.importance_samples).parameters) == ["self", "rays", "samples", "weights",
                                                                                          "num_importance", "kw"]
    rays = lp.Rays(directions=torch.ones(2, 3), origins=torch.zeros(2, 3), grid_idx=torch.zeros(2, dtype=torch.long),
                   near=torch.zeros(2), far=torch.ones(2))
    d, w = torch.rand(2, 4).cumsum(-1), torch.rand(2, 4)
    # there is no CPU path: tensors that pass every check still need a GPU
    with pytest.raises(_lib.LightplaneHipError, match="GPU only"):
        lp.importance_samples(rays, d, w, 3)
    with pytest.raises(AssertionError, match="Rays object"):
        lp.importance_samples(None, d, w, 3)
    with pytest.raises(AssertionError, match="2 to 2048"):
        lp.importance_samples(rays, d[:, :1], w[:, :1], 3)
    with pytest.raises(AssertionError, match="2 to 2048"):
        lp.importance_samples(rays, torch.zeros(2, 2049), torch.zeros(2, 2049), 3)
    for n in (0, 2049):
        with pytest.raises(AssertionError, match="num_importance"):
            lp.importance_samples(rays, d, w, n)
    with pytest.raises(AssertionError, match="weights"):
        lp.importance_samples(rays, d, w[:, :3], 3)
    for pad in (0.0, -1e-5, float("inf"), float("nan")):
        with pytest.raises(AssertionError, match="pad"):
            lp.importance_samples(rays, d, w, 3, pad=pad)
    with pytest.raises(AssertionError, match="jitter"):
        lp.importance_samples(rays, d, w, 3, jitter=torch.rand(2, 4))
    with pytest.raises(AssertionError, match="rays.origins"):
        lp.importance_samples(rays, torch.cat([d, d]), torch.cat([w, w]), 3)
    with pytest.raises(AssertionError, match="float32"):
        lp.importance_samples(rays, d.double(), w, 3)
    with pytest.raises(AssertionError, match="float32"):
        lp.importance_samples(rays, d, w, 3, jitter=torch.rand(2, 3).double())


def test_null_arguments_are_refused():
    L = _lib.lib()
    for name in _lib.IMPORTANCE_EXPORTS:
        assert getattr(L, name)(None, None) == -3 and _err().startswith("args is NULL"), name
        for f in REQUIRED[name]:
            a = _args()
            setattr(a, f, None)
            assert _call(name, a) == -3 and _err().startswith(f"{f} is NULL"), (name, f, _err())


def test_optional_pointers_may_be_null():
    """what a call does not need may be NULL: the first failing check is then another one; with no rays every check is passed"""
    a = _args(n_rays=0)
    for f in FIELDS:
        setattr(a, f, None)
    for name in _lib.IMPORTANCE_EXPORTS:
        assert _call(name, a) == 0, (name, _err())
        assert _call(name, _args(n_rays=0)) == 0, (name, _err())
        assert _call(name, _args(n_rays=0, n_samples=2048, n_importance=2048, include_coarse=0)) == 0, (name, _err())
    for name in _lib.IMPORTANCE_EXPORTS:
        a = _args()
        for f in FIELDS:
            if f not in REQUIRED[name]:
                setattr(a, f, None)
        last = REQUIRED[name][-1]
        setattr(a, last, None)
        assert _call(name, a) == -3 and _err().startswith(f"{last} is NULL"), (name, _err())


def test_under_aligned_pointers_are_refused():
    for off in (4, 8, 12):
        for name in _lib.IMPORTANCE_EXPORTS:
            for n_rays in (3, 0):  # (whatever n_rays is)
                for f in FIELDS:
                    a = _args(n_rays=n_rays)
                    setattr(a, f, FAKE + 40 * STEP + off)
                    assert _call(name, a) == -1 and _err().startswith(f"{f} = ") and "16-byte aligned" in _err(), (name, f, off, _err())


def test_malformed_shapes_are_refused():
    for name in _lib.IMPORTANCE_EXPORTS:
        assert _call(name, _args(n_rays=-1)) == -1 and _err().startswith("n_rays -1"), _err()
        for s in (1, 0, -3):
            assert _call(name, _args(n_samples=s)) == -1 and _err().startswith(f"n_samples {s} < 2"), _err()
        for n in (0, -1):
            assert _call(name, _args(n_importance=n)) == -1 and _err().startswith(f"n_importance {n} < 1"), _err()
        for pad in (0.0, -1e-5, float("inf"), float("-inf"), float("nan")):
            assert _call(name, _args(pad=pad)) == -1 and _err().startswith("pad "), (pad, _err())
        assert _call(name, _args(n_samples=2049)) == -2 and _err().startswith("n_samples 2049 > 2048"), _err()
        assert _call(name, _args(n_importance=2049)) == -2 and _err().startswith("n_importance 2049 > 2048"), _err()
        assert _call(name, _args(n_rays=1 << 19, n_samples=2048, n_importance=2048)) == -2 and _err().startswith("n_rays") and "2^31" in _err(), _err()
        a = _args(n_rays=(1 << 19) - 1, n_samples=2048, n_importance=2048)  # (below 2^31: the next check refuses)
        a.directions = None
        assert _call(name, a) == -3 and _err().startswith("directions is NULL"), _err()


def test_the_case_table_covers_the_agreed_shapes():
    assert IC.RS == (1, 63, 130) and IC.SS == (2, 3, 63, 64, 65, 131) and IC.NS == (1, 2, 63, 64, 65, 130)
    assert IC.REGIMES == ("transparent", "opaque", "mixed", "duplicates") and IC.LIMIT_CASE[1:] == (2048, 2048)
    assert {(c[1], c[2]) for c in IC.CASES} == {(S, N) for S in IC.SS for N in IC.NS} and {c[0] for c in IC.CASES} == set(IC.RS)
    assert IC.B == 4 * 2.0 ** -24 and IC.bar_a(64) == 4 * 64 * 2.0 ** -24
    c = IC.inputs(130, 65, 64, "transparent")
    assert 0.5e-4 < float(c["weights"].mean()) < 2e-4 and bool((c["depths"][:, 1:] > c["depths"][:, :-1]).all())
    assert bool((c["jitter"] >= 0).all()) and bool((c["jitter"] < 1).all())
    c = IC.inputs(130, 65, 64, "opaque")
    assert bool(((c["weights"] == 0.97).sum(-1) == 1).all()) and abs(float(c["weights"].min()) - 1e-6) < 1e-12
    c = IC.inputs(130, 65, 64, "mixed")
    assert float(c["weights"][1::3].abs().max()) == 0.0 and float(c["weights"][0, 32:].abs().max()) == 0.0 and float(c["weights"][0, :32].min()) > 0
    assert bool(torch.isnan(c["weights"][2::3, 21]).all()) and bool((c["weights"][2::3, 0] == -1).all())
    c = IC.inputs(130, 65, 64, "duplicates")
    e = IC.edges(c["depths"])
    assert bool(((e[:, 1:] == e[:, :-1]).sum(-1) == 2).all())  # two zero-width bins
    assert bool((c["depths"][:, 1:] >= c["depths"][:, :-1]).all())
    e = IC.edges(IC.inputs(63, 2, 2, "duplicates")["depths"])
    assert bool(((e[:, 1:] == e[:, :-1]).sum(-1) == 2).all())


@pytest.mark.parametrize("regime", IC.REGIMES)
def test_the_bar_is_one_the_definition_meets_in_fp32(regime):
    """the test of the test: the fp32 restatement of the definition, held to the bar the kernel is held to; its margin is printed"""
    worst = (0.0, None)
    for S in IC.HOST_SS:
        for N in IC.HOST_NS:
            c = IC.inputs(IC.HOST_R, S, N, regime)
            for jitter in (None, c["jitter"]):
                t32, _ = IC.new_depths(c["depths"], c["weights"], N, IC.PAD, jitter, torch.float32)
                assert t32.dtype == torch.float32
                ex, _ = IC.bar_excess(t32, c["depths"], c["weights"], N, IC.PAD, jitter)
                worst = max(worst, (ex, (S, N, jitter is not None)))
                assert ex <= 4.0, f"S={S} N={N}: the fp32 restatement is {ex:.3f} S 2^-24 outside the B window (the bar: 4)"
                # fp64 against itself: inside the B window with room to spare
                t64, _ = IC.new_depths(c["depths"], c["weights"], N, IC.PAD, jitter, torch.float64)
                assert IC.bar_excess(t64, c["depths"], c["weights"], N, IC.PAD, jitter)[0] <= 1e-6
                # monotone in k and inside the ray's span, exactly, in both precisions
                for t, d in ((t32, c["depths"]), (t64, c["depths"].double())):
                    assert bool((t[:, 1:] >= t[:, :-1]).all()) and bool((t >= d[:, :1]).all()) and bool((t <= d[:, -1:]).all())
    print(f"{regime}: worst excess of the fp32 restatement over the B window {worst[0]:.3f} S 2^-24 at (S, N, jitter) = {worst[1]} (the bar: 4)")


def test_a_plain_relative_bar_would_refuse_the_definition():
    """why the bar is not 'max |err| / max |t| <= 1e-4': the correct fp32 restatement misses it where a bin is nearly empty"""
    worst = 0.0
    for S in IC.HOST_SS:
        c = IC.inputs(IC.HOST_R, S, 257, "opaque")
        t32, _ = IC.new_depths(c["depths"], c["weights"], 257, IC.PAD, None, torch.float32)
        t64, _ = IC.new_depths(c["depths"], c["weights"], 257, IC.PAD, None, torch.float64)
        worst = max(worst, float((t32.double() - t64).abs().max() / t64.abs().max()))
    print(f"opaque regime, fp32 restatement against fp64: max |err| / max |t| = {worst:.3e}")
    assert worst > 1e-6  # (many fp32 ulps: the slope of the inverse CDF, not a defect)


@pytest.mark.parametrize("regime", IC.REGIMES)
def test_histogram_of_many_samples_is_the_mass_of_the_bins(regime):
    N = 4096
    for S in (2, 3, 65, 131):
        c = IC.inputs(5, S, N, regime)
        for jitter in (None, c["jitter"]):
            _, j = IC.new_depths(c["depths"], c["weights"], N, IC.PAD, jitter, torch.float64)
            p, C = IC.masses(c["weights"], IC.PAD, torch.float64)
            share = torch.zeros_like(p).scatter_add_(1, j, torch.ones_like(j, dtype=torch.float64)) / N
            err = float((share - p / C[:, -1:]).abs().max())
            # a bin's interval of the CDF holds every stratum it covers and may hold the one or two it cuts: the centres of the strata
            # (deterministic) are within one sample of the mass, jittered ones within two
            bound = (1.0 if jitter is None else 2.0) / N
            assert err <= bound + 1e-12, f"{regime} S={S}: a bin's share of {N} samples is {err:.3e} from its mass (the bound: {bound:.3e})"


def test_all_zero_rows_get_the_same_mass_in_every_bin():
    """A ray of all-zero weights: ``p_j = pad`` in every bin, so the new depths are uniform over the BINS -- the closed form
    ``equal_mass_depths``.  That is uniform in depth, ``d_0 + u_k (d_{S-1} - d_0)``, exactly where all bins have one width, which with
    edges at the midpoints (two half-width end bins) means S = 2; the same check runs on the kernel (tests/test_gpu_importance.py)."""
    for S in (2, 3, 65, 131):
        for N in (1, 64, 257):
            c = IC.inputs(33, S, N, "mixed")
            d = c["depths"][1::3].double()
            for jitter in (None, c["jitter"]):
                jz = None if jitter is None else jitter[1::3]
                t, _ = IC.new_depths(c["depths"], c["weights"], N, IC.PAD, jitter, torch.float64)
                want = IC.equal_mass_depths(c["depths"][1::3], N, jz)
                assert float((t[1::3] - want).abs().max()) <= 1e-9 * float(want.abs().max())
                if S == 2:
                    uniform = d[:, :1] + IC.targets(d.shape[0], N, jz, torch.float64) * (d[:, -1:] - d[:, :1])
                    assert float((t[1::3] - uniform).abs().max()) <= 1e-9 * float(uniform.abs().max())


def test_merge_deltas_and_points_of_the_definition():
    c = IC.inputs(7, 5, 4, "transparent")
    pts, d, dl = IC.resample(c["origins"], c["directions"], c["depths"], c["weights"], 4)
    assert pts.shape == (7, 9, 3) and d.shape == dl.shape == (7, 9) and bool((d[:, 1:] >= d[:, :-1]).all())
    assert torch.equal(dl[:, 0], dl[:, 1]) and torch.equal(dl[:, 1:], d[:, 1:] - d[:, :-1])
    _, d1, dl1 = IC.resample(c["origins"], c["directions"], c["depths"], c["weights"], 1, include_coarse=False)
    assert d1.shape == (7, 1) and bool((dl1 == 1).all())
    assert math.isclose(float(pts[2, 3, 1]), float(d[2, 3] * c["directions"][2, 1].double() + c["origins"][2, 1].double()), rel_tol=1e-14)

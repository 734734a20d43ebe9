"""CPU tests of the host side of the distortion and the interlevel loss: the four lp_distortion_* / lp_interlevel_* symbols and their two
ABI structs, the header of their own (include/lightplane_hip_losses.h), every argument check (each returns its code and a message that
begins with the field, before anything touches a device), the Python surface, and the definitions' own properties
(tests/ray_loss_cases.py): the O(S) forms the kernels use equal autograd of the definitions in fp64, their fp32 restatement is inside
the bars the kernels are held to, and the interlevel cases violate the bound where they are meant to."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib, ray_losses
from tests import ray_loss_cases as LC

FAKE = 0x10000  # 16-byte-aligned non-NULL "device pointers": no check dereferences them, and every call below fails a check
STEP = 0x1000000  # (or has no rays to launch for)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lightplane_hip_losses.h")
EXPORTS = ("lp_distortion_forward", "lp_distortion_backward", "lp_interlevel_forward", "lp_interlevel_backward")
FIELDS = {"d": ("weights", "depths", "deltas", "grad_loss", "loss", "grad_weights", "grad_depths", "grad_deltas"),
          "i": ("weights", "depths", "proposal_weights", "proposal_depths", "grad_loss", "loss", "grad_proposal_weights")}
REQUIRED = {"lp_distortion_forward": ("weights", "depths", "deltas", "loss"),
            "lp_distortion_backward": ("weights", "depths", "deltas"),
            "lp_interlevel_forward": ("weights", "depths", "proposal_weights", "proposal_depths", "loss"),
            "lp_interlevel_backward": ("weights", "depths", "proposal_weights", "proposal_depths", "grad_proposal_weights")}
BUILD_INFO_KEYS = ["version", "src_hash", "test_hooks", "tuned_bwd", "loop_bwd_deep", "loop_bwd_shallow", "mlp_splatter_bwd",
                   "loop_fwd_stream", "grid_tv", "grid_resample", "scaffold", "points", "ray_clip", "point_grid", "mesh", "forward", "flags"]


def _kind(name):
    return "d" if "distortion" in name else "i"


def _args(name, n_rays=3, n_samples=5, n_proposal=4, eps=1e-7):
    if _kind(name) == "d":
        a = _lib.LpDistortionArgs()
    else:
        a = _lib.LpInterlevelArgs()
        a.n_proposal, a.eps = n_proposal, eps
    a.n_rays, a.n_samples = n_rays, n_samples
    for i, f in enumerate(FIELDS[_kind(name)]):
        setattr(a, f, FAKE + i * STEP)
    return a


def _err():
    return _lib.lib().lp_last_error().decode()


def _call(name, a):
    return getattr(_lib.lib(), name)(ctypes.byref(a), None)


# ------------------------------------------------------------------------------------------------------------------------------
# symbols, structs, header
# ------------------------------------------------------------------------------------------------------------------------------

def test_symbols_structs_and_tables():
    L = _lib.lib()
    assert _lib.LOSSES_EXPORTS == EXPORTS
    for name in EXPORTS:
        assert hasattr(L, name), f"{name} not exported by liblightplane_hip.so"
        # (the tables of the other three headers stay as they are)
        assert name not in _lib.EXPORTS and name not in _lib.SAMPLES_EXPORTS and name not in _lib.IMPORTANCE_EXPORTS
    assert L.lp_abi_sizeof(24) == ctypes.sizeof(_lib.LpDistortionArgs) == 80
    assert L.lp_abi_sizeof(26) == ctypes.sizeof(_lib.LpInterlevelArgs) == 80
    for which in (23, 25, 27, 28, 99):
        assert L.lp_abi_sizeof(which) == -1, which
    assert L.lp_abi_sizeof(22) == ctypes.sizeof(_lib.LpImportanceArgs)
    assert L.lp_version() == 207  # additive: no version change
    assert list(_lib.build_info()) == BUILD_INFO_KEYS  # no new key
    from lightplane_amd.csrc import build as B
    assert _lib.build_info()["src_hash"] == B.source_hash()
    assert any(h.endswith("lightplane_hip_losses.h") for h in B.PUBLIC_HEADERS) and "lp_ray_losses.hip" in B.SOURCES
    assert any(h.endswith("lightplane_hip_losses.h") for h in B.HEADERS)


def test_header_declares_the_bound_symbols_and_is_plain_c(tmp_path):
    text = open(HEADER).read()
    assert tuple(re.findall(r"^int (lp_\w+)\(", text, re.M)) == EXPORTS
    assert '#include "lightplane_hip.h"' in text
    assert int(re.search(r"#define LP_RAY_LOSS_MAX (\d+)", text).group(1)) == _lib.LP_RAY_LOSS_MAX == 2048
    # every buffer says whether it is written entirely or read; none is accumulated into
    for f in set(FIELDS["d"]) | set(FIELDS["i"]):
        line = [ln for ln in text.splitlines() if re.search(rf"\bfloat\* {f};", ln)]
        assert line and all("WRITTEN entirely" in ln or "read" in ln for ln in line), f
    for other in ("lightplane_hip.h", "lightplane_hip_samples.h", "lightplane_hip_importance.h"):
        declared = re.findall(r"^int (lp_\w+)\(", open(os.path.join(ROOT, "include", other)).read(), re.M)
        assert not set(EXPORTS) & set(declared), other
    assert '#include "../../include/lightplane_hip_losses.h"' in open(os.path.join(ROOT, "lightplane_amd", "csrc", "lp_host.h")).read()
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None, "a C compiler (cc or gcc) is needed: the header has to pass it as plain C"
    subprocess.run([cc, "-x", "c", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", HEADER], check=True)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "lightplane_hip_losses.h"\nint main(void){printf("%zu %zu\\n", '
                   'sizeof(LpDistortionArgs), sizeof(LpInterlevelArgs)); return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    sizes = [int(v) for v in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE).stdout.split()]
    assert sizes[0] == ctypes.sizeof(_lib.LpDistortionArgs) == _lib.lib().lp_abi_sizeof(24)
    assert sizes[1] == ctypes.sizeof(_lib.LpInterlevelArgs) == _lib.lib().lp_abi_sizeof(26)


# ------------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------------

def test_null_arguments_are_refused():
    L = _lib.lib()
    for name in EXPORTS:
        assert getattr(L, name)(None, None) == -3 and _err().startswith("args is NULL"), name
        for f in REQUIRED[name]:
            a = _args(name)
            setattr(a, f, None)
            assert _call(name, a) == -3 and _err().startswith(f"{f} is NULL"), (name, f, _err())


def test_optional_pointers_may_be_null():
    """what a call does not need may be NULL (grad_loss: ones); with no rays every check is passed and nothing is launched; a
    distortion backward that is asked for no gradient launches nothing either"""
    for name in EXPORTS:
        a = _args(name, n_rays=0)
        for f in FIELDS[_kind(name)]:
            setattr(a, f, None)
        assert _call(name, a) == 0, (name, _err())
        assert _call(name, _args(name, n_rays=0)) == 0, (name, _err())
        assert _call(name, _args(name, n_rays=0, n_samples=2048, n_proposal=2048)) == 0, (name, _err())
        a = _args(name)
        for f in FIELDS[_kind(name)]:
            if f not in REQUIRED[name]:
                setattr(a, f, None)
        if name == "lp_distortion_backward":
            assert _call(name, a) == 0, _err()  # (no gradient asked for: LP_OK without a launch)
        last = REQUIRED[name][-1]
        setattr(a, last, None)
        assert _call(name, a) == -3 and _err().startswith(f"{last} is NULL"), (name, _err())


def test_under_aligned_pointers_are_refused():
    for off in (4, 8, 12):
        for name in EXPORTS:
            for n_rays in (3, 0):  # (whatever n_rays is)
                for f in FIELDS[_kind(name)]:
                    a = _args(name, n_rays=n_rays)
                    setattr(a, f, FAKE + 40 * STEP + off)
                    assert _call(name, a) == -1 and _err().startswith(f"{f} = ") and "16-byte aligned" in _err(), (name, f, off, _err())


def test_malformed_shapes_are_refused():
    for name in EXPORTS:
        least = 1 if _kind(name) == "d" else 2
        assert _call(name, _args(name, n_rays=-1)) == -1 and _err().startswith("n_rays -1"), _err()
        for s in (least - 1, -3):
            assert _call(name, _args(name, n_samples=s)) == -1 and _err().startswith(f"n_samples {s} < {least}"), _err()
        assert _call(name, _args(name, n_samples=2049)) == -2 and _err().startswith("n_samples 2049 > 2048"), _err()
        assert _call(name, _args(name, n_rays=1 << 20, n_samples=2048)) == -2 and _err().startswith("n_rays") and "2^31" in _err(), _err()
        a = _args(name, n_rays=(1 << 20) - 1, n_samples=2048, n_proposal=2048)  # (below 2^31: the next check refuses)
        a.weights = None
        assert _call(name, a) == -3 and _err().startswith("weights is NULL"), _err()
        if _kind(name) == "d":
            a = _args(name, n_samples=1)
            a.depths = None
            assert _call(name, a) == -3 and _err().startswith("depths is NULL"), _err()  # (a single sample is a shape)
            continue
        for p in (1, 0, -1):
            assert _call(name, _args(name, n_proposal=p)) == -1 and _err().startswith(f"n_proposal {p} < 2"), _err()
        for eps in (0.0, -1e-7, float("inf"), float("-inf"), float("nan")):
            assert _call(name, _args(name, eps=eps)) == -1 and _err().startswith("eps "), (eps, _err())
        assert _call(name, _args(name, n_proposal=2049)) == -2 and _err().startswith("n_proposal 2049 > 2048"), _err()
        # the longer of the two rows counts
        assert _call(name, _args(name, n_rays=1 << 20, n_samples=2, n_proposal=2048)) == -2 and "2^31" in _err(), _err()


# ------------------------------------------------------------------------------------------------------------------------------
# Python surface
# ------------------------------------------------------------------------------------------------------------------------------

def test_python_surface():
    assert "distortion_loss" in lp.__all__ and lp.distortion_loss is ray_losses.distortion_loss
    assert "interlevel_loss" in lp.__all__ and lp.interlevel_loss is ray_losses.interlevel_loss
    assert list(inspect.signature(lp.distortion_loss).parameters) == ["weights", "depths", "deltas"]
    sig = inspect.signature(lp.interlevel_loss)
    assert list(sig.parameters) == ["weights", "depths", "proposal_weights", "proposal_depths", "eps"]
    assert sig.parameters["eps"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["eps"].default == 1e-7
    assert "far - near" in lp.distortion_loss.__doc__  # (normalised distances are the caller's division)
    w, d = torch.rand(2, 4), torch.rand(2, 4).cumsum(-1)
    pw, pd = torch.rand(2, 3), torch.rand(2, 3).cumsum(-1)
    # there is no CPU path: tensors that pass every check still need a GPU
    with pytest.raises(_lib.LightplaneHipError, match="GPU only"):
        lp.distortion_loss(w, d, d)
    with pytest.raises(_lib.LightplaneHipError, match="GPU only"):
        lp.interlevel_loss(w, d, pw, pd)
    with pytest.raises(AssertionError, match="1 to 2048"):
        lp.distortion_loss(torch.zeros(2, 2049), torch.zeros(2, 2049), torch.zeros(2, 2049))
    with pytest.raises(AssertionError, match="1 to 2048"):
        lp.distortion_loss(torch.zeros(2, 0), torch.zeros(2, 0), torch.zeros(2, 0))
    with pytest.raises(AssertionError, match="weights"):
        lp.distortion_loss(w[0], d, d)
    with pytest.raises(AssertionError, match="depths"):
        lp.distortion_loss(w, d[:, :3], d)
    with pytest.raises(AssertionError, match="deltas"):
        lp.distortion_loss(w, d, d[:1])
    with pytest.raises(AssertionError, match="float32"):
        lp.distortion_loss(w, d.double(), d)
    for bad in (w[:, :1], torch.zeros(2, 2049)):
        with pytest.raises(AssertionError, match="2 to 2048"):
            lp.interlevel_loss(bad, bad, pw, pd)
        with pytest.raises(AssertionError, match="2 to 2048"):
            lp.interlevel_loss(w, d, bad, bad)
    with pytest.raises(AssertionError, match="depths"):
        lp.interlevel_loss(w, d[:, :3], pw, pd)
    with pytest.raises(AssertionError, match="proposal_weights"):
        lp.interlevel_loss(w, d, pw[:1], pd)
    with pytest.raises(AssertionError, match="proposal_depths"):
        lp.interlevel_loss(w, d, pw, pd[:, :2])
    for eps in (0.0, -1e-7, float("inf"), float("nan")):
        with pytest.raises(AssertionError, match="eps"):
            lp.interlevel_loss(w, d, pw, pd, eps=eps)
    with pytest.raises(AssertionError, match="float32"):
        lp.interlevel_loss(w, d, pw.double(), pd)


# ------------------------------------------------------------------------------------------------------------------------------
# the definitions
# ------------------------------------------------------------------------------------------------------------------------------

def _rel(name, got, want):
    scale = max(float(want.abs().max()), 1e-300)
    err = float((got.double() - want).abs().max()) / scale
    print(f"{name}: max |err| / max |ref| = {err:.3e}")
    return err


def test_the_case_tables_cover_the_agreed_shapes():
    assert LC.RS == (1, 63, 130) and LC.DIST_SS == (1, 2, 3, 63, 64, 65, 131) and LC.INTER_SS == (2, 3, 63, 64, 65, 131)
    assert {c[1] for c in LC.DIST_CASES} == set(LC.DIST_SS) and {c[0] for c in LC.DIST_CASES} == set(LC.RS)
    assert LC.DIST_LIMIT == (3, 2048) and LC.INTER_LIMIT == (3, 2048, 2048)
    assert {S for S, _ in LC.INTER_PAIRS} == {P for _, P in LC.INTER_PAIRS} == set(LC.INTER_SS)
    assert len(set(LC.INTER_PAIRS)) == len(LC.INTER_PAIRS) and {c[0] for c in LC.INTER_CASES} == set(LC.RS)
    for rel in (lambda s, p: s < p, lambda s, p: s == p, lambda s, p: s > p):
        assert sum(rel(S, P) for S, P in LC.INTER_PAIRS) >= 4
    assert LC.bar_sum(64) == 4 * 64 * 2.0 ** -24 and LC.TOL == 1e-4
    c = LC.distortion_inputs(130, 65, "transparent")
    assert 0.5e-4 < float(c["weights"].mean()) < 2e-4 and bool((c["depths"][:, 1:] > c["depths"][:, :-1]).all())
    c = LC.distortion_inputs(130, 65, "opaque")
    assert bool(((c["weights"] == 0.97).sum(-1) == 1).all())
    c = LC.distortion_inputs(130, 65, "mixed")
    assert float(c["weights"][1::3].abs().max()) == 0.0 and float(c["weights"][0, 32:].abs().max()) == 0.0 and float(c["weights"][0, :32].min()) > 0
    assert bool((c["weights"][2::3, 21] < 0).all())
    c = LC.distortion_inputs(130, 65, "duplicates")
    assert bool(((c["depths"][:, 1:] == c["depths"][:, :-1]).sum(-1) == 4).all()) and bool((c["depths"][:, 1:] >= c["depths"][:, :-1]).all())
    for regime in LC.NONNEG:
        c = LC.distortion_inputs(63, 64, regime)
        assert float(c["weights"].min()) >= 0 and float(c["deltas"].min()) > 0


@pytest.mark.parametrize("S", [1, 2, 65, 131])
def test_distortion_scan_forms_equal_autograd_of_the_pair_definition(S):
    """the O(S) forms of the header against fp64 autograd of the O(S^2) definition, tied depths included: 1e-12 of max"""
    for regime in LC.DIST_REGIMES:
        c = LC.distortion_inputs(7, S, regime)
        ref = LC.distortion_oracle(c["weights"], c["depths"], c["deltas"])
        got = LC.distortion_scan(c["weights"], c["depths"], c["deltas"])
        for key, a, b in zip(("loss", "d weights", "d depths", "d deltas"), got, ref):
            assert _rel(f"S={S} {regime} {key}", a, b) <= 1e-12
    # mip-NeRF 360's absolute-value form, for sorted depths
    c = LC.distortion_inputs(7, S, "mixed")
    w, d = c["weights"].double(), c["depths"].double()
    absform = (w[:, :, None] * w[:, None, :] * (d[:, :, None] - d[:, None, :]).abs()).sum((1, 2)) + (w * w * c["deltas"].double()).sum(-1) / 3
    assert _rel(f"S={S} |d_i - d_j| form", LC.distortion_pairs(w, d, c["deltas"].double()), absform) <= 1e-12
    # translation invariance and homogeneity: L(w, a d + b, a delta) = a L(w, d, delta)
    scaled = LC.distortion_pairs(w, 3.0 * d + 11.0, 3.0 * c["deltas"].double())
    assert _rel(f"S={S} homogeneity", scaled, 3.0 * LC.distortion_pairs(w, d, c["deltas"].double())) <= 1e-12


@pytest.mark.parametrize("S", [1, 2, 3, 63, 64, 65, 131, 2048])
def test_distortion_bars_are_ones_the_fp32_restatement_meets(S):
    """the test of the test: the forms in fp32 (torch's own summation order), held to the bars the kernel is held to"""
    for regime in LC.DIST_REGIMES:
        c = LC.distortion_inputs(3, S, regime)
        ref = LC.distortion_oracle(c["weights"], c["depths"], c["deltas"])
        got = LC.distortion_scan(c["weights"], c["depths"], c["deltas"], torch.float32)
        assert got[0].dtype == torch.float32
        for key, a, b in zip(("loss", "d weights", "d depths", "d deltas"), got, ref):
            assert _rel(f"S={S} {regime} fp32 {key}", a, b) <= LC.TOL
        if regime in LC.NONNEG:
            for key, a, b in (("loss", got[0], ref[0]), ("d weights", got[1], ref[1])):
                worst = float(((a.double() - b).abs() / b.abs().clamp(min=1e-300)).max()) / (S * LC.EPS24)
                print(f"S={S} {regime} fp32 {key}: worst entry {worst:.3f} S 2^-24 relative (the bar: 4)")
                assert bool(((a.double() - b).abs() <= LC.bar_sum(S) * b.abs()).all())


@pytest.mark.parametrize("S,P", [(2, 2), (2, 65), (65, 2), (65, 131), (131, 65), (131, 131)])
def test_interlevel_scan_forms_equal_autograd_of_the_definition(S, P):
    for regime in LC.INTER_REGIMES:
        if not LC.interlevel_possible(S, P, regime):
            continue
        c = LC.interlevel_inputs(7, S, P, regime)
        four = (c["weights"], c["depths"], c["proposal_weights"], c["proposal_depths"])
        loss, grad, _ = LC.interlevel_oracle(*four)
        got = LC.interlevel_scan(*four)
        assert _rel(f"S={S} P={P} {regime} loss", got[0], loss) <= 1e-12 or float(loss.abs().max()) == 0.0 == float(got[0].abs().max())
        assert _rel(f"S={S} P={P} {regime} d proposal_weights", got[1], grad) <= 1e-12 or float(grad.abs().max()) == 0.0 == float(got[1].abs().max())
        # lo and hi do not decrease along the ray: the gradient's range of cells is contiguous
        lo, hi = LC.touching(c["depths"], c["proposal_depths"])
        assert bool((lo[:, 1:] >= lo[:, :-1]).all()) and bool((hi[:, 1:] >= hi[:, :-1]).all()) and bool((hi >= lo).all())
        # the brute-force overlap test: proposal cell j touches target cell k iff the closed cells share a point, counted from the
        # first edge at or below the cell's start
        e, eh = LC.edges(c["depths"]), LC.edges(c["proposal_depths"])
        j = torch.arange(P)[None, None, :]
        touch = (lo[:, :, None] <= j) & (j < hi[:, :, None])
        plain = (eh[:, None, :-1] <= e[:, 1:, None]) & (eh[:, None, 1:] > e[:, :-1, None])
        assert bool((touch >= plain).all())  # every overlapping cell is counted


def test_interlevel_fp32_prefix_sums_are_why_the_kernel_holds_them_in_fp64():
    """a figure, printed: the gradient from fp32 prefix sums at S = P = 2048 against the fp64 definition"""
    c = LC.interlevel_inputs(3, 2048, 2048, "violating")
    four = (c["weights"], c["depths"], c["proposal_weights"], c["proposal_depths"])
    _, grad, _ = LC.interlevel_oracle(*four)
    e32 = _rel("fp32 prefix sums, S = P = 2048", LC.interlevel_scan(*four, dtype=torch.float32)[1], grad)
    e64 = _rel("fp64 prefix sums, S = P = 2048", LC.interlevel_scan(*four, dtype=torch.float64)[1], grad)
    assert e64 <= 1e-12 < e32


@pytest.mark.parametrize("R,S,P", LC.INTER_CASES)
def test_interlevel_cases_violate_where_they_should(R, S, P):
    """the condition of the GPU test, on the CPU: covered cases have no violated cell, a loss of exactly 0 and a gradient of exactly 0;
    in every other regime at least 10 % of all cells have w_k > bound_k"""
    for regime in LC.INTER_REGIMES:
        if not LC.interlevel_possible(S, P, regime):
            continue
        loss, grad, violated = LC.interlevel_case(R, S, P, regime)["ref"]
        share = float(violated.double().mean())
        print(f"R={R} S={S} P={P} {regime}: {100 * share:.1f} % of the cells violated")
        if regime == "covered":
            assert share == 0.0 and float(loss.abs().max()) == 0.0 and float(grad.abs().max()) == 0.0
        else:
            assert share >= 0.10
            # (the oracle's gradient is autograd's difference of two suffix sums: zero up to its rounding)
            assert float(loss.min()) >= 0 and float(loss.max()) > 0 and float(grad.max()) <= 1e-12 * float(grad.abs().max())
            # (rows of fewer than 8 depths, all equal: every edge is the same point, no proposal cell bounds anything)
            assert float(grad.min()) < 0 or (regime == "duplicates" and min(S, P) < 8)
        c = LC.interlevel_case(R, S, P, regime)
        for key in ("depths", "proposal_depths"):
            assert bool((c[key][:, 1:] >= c[key][:, :-1]).all()), key
        if regime == "disjoint":
            assert bool((c["proposal_depths"][:, 0] > c["depths"][:, 0]).all()) and bool((c["proposal_depths"][:, -1] < c["depths"][:, -1]).all())
        if regime == "contains":
            both = torch.cat([c["depths"], c["proposal_depths"]], 1).sort(1).values
            assert bool((both[:, 1:] == both[:, :-1]).sum(-1).ge(P).all())  # every proposal depth is a target depth
            assert torch.equal(c["depths"][:, 0], c["proposal_depths"][:, 0]) and torch.equal(c["depths"][:, -1], c["proposal_depths"][:, -1])

"""Every entry point of the C ABI answers the malformed blocks of tests/api_error_cases.py as recorded in tests/golden/api_errors.json:
the same return code and the same lp_last_error() text, byte for byte.  CPU only -- no case reaches a kernel.  The fixture is rewritten
with scripts/record_api_errors.py when an answer is meant to change."""
import json
import os

import pytest

from lightplane_amd import _lib
from tests import api_error_cases as A

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "api_errors.json")) as _f:
    FIXTURE = json.load(_f)

LP_OK, LP_EINVAL, LP_EUNSUPPORTED, LP_ENULL = 0, -1, -2, -3
# lp_build_info() of the library before its keys moved into a table
BUILD_INFO_KEYS = ("version", "src_hash", "test_hooks", "tuned_bwd", "loop_bwd_deep", "loop_bwd_shallow", "mlp_splatter_bwd", "loop_fwd_stream",
                   "grid_tv", "grid_resample", "scaffold", "points", "ray_clip", "point_grid", "mesh", "forward", "flags")


def test_the_fixture_and_the_table_hold_the_same_cases():
    assert sorted(FIXTURE) == sorted(A.CASES)


def test_every_entry_point_is_in_the_table_and_is_refused_at_least_once():
    L = _lib.lib()
    assert set(A.ENTRY_POINTS) <= set(_lib.EXPORTS) | {"lp_renderer_forward_workspace_bytes", "lp_grid_tv_workspace_bytes",
                                                       "lp_scaffold_workspace_bytes", "lp_mesh_workspace_bytes"}
    silent = {"lp_version", "lp_last_error", "lp_build_info", "lp_abi_sizeof"}   # (nothing to refuse, or no message)
    assert set(_lib.EXPORTS) - silent <= set(A.ENTRY_POINTS)
    for name in A.ENTRY_POINTS:
        assert hasattr(L, name), name
        codes = [FIXTURE[cid][0] for cid in FIXTURE if A.entry_point(cid) == name]
        assert any(c < 0 for c in codes), f"no refused case for {name}"


def test_no_recorded_case_reached_a_launch():
    """a launcher answers LP_OK (an empty batch) or one of the three argument errors: a positive code would be a hipError_t, i.e. a case that
    got past the checks with rays to work on"""
    for cid, (code, msg) in FIXTURE.items():
        if A.entry_point(cid) in A.QUERIES:
            assert code >= LP_ENULL, cid
        else:
            assert code in (LP_OK, LP_EINVAL, LP_EUNSUPPORTED, LP_ENULL), (cid, code, msg)
        assert (msg == "") == (code >= 0), (cid, code, msg)


@pytest.mark.parametrize("entry", A.ENTRY_POINTS)
def test_codes_and_messages_are_the_recorded_ones(entry):
    cids = [cid for cid in A.CASES if A.entry_point(cid) == entry]
    assert cids
    wrong = {cid: (FIXTURE[cid], got) for cid in cids for got in [A.run(cid)] if got != FIXTURE[cid]}
    assert not wrong, "\n".join(f"{cid}: recorded {want}, got {got}" for cid, (want, got) in wrong.items())


def test_build_info_parses_and_keeps_its_keys():
    text = _lib.lib().lp_build_info().decode()
    info = json.loads(text)
    assert tuple(info) == BUILD_INFO_KEYS          # (and in this order: the text is the same byte for byte)
    assert info["version"] == _lib.lib().lp_version() and isinstance(info["forward"], str) and isinstance(info["mesh"], dict)
    assert text.startswith(f'{{"version": {info["version"]}, "src_hash": "{info["src_hash"]}", "test_hooks": ')
    assert text.endswith(', "mesh": ' + json.dumps(info["mesh"]) + ', "forward": "bf16x3 (three exact bf16 limbs per fp32 operand, six limb products, '
                         'fp32 accumulation) on v_mfma_f32_32x32x16_bf16; generic kernels: fp32 FMA", "flags": ' + json.dumps(info["flags"]) + "}")

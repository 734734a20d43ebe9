"""The workgroup count of every launcher (csrc/lp_launch.h: workgroup_count, behind launch_blocks of lp_host.h), checked on the CPU.

tests/host/launch_blocks_check.cpp is a stand-alone program around the very function the launchers call.  It is built here with the
address and undefined-behaviour sanitizers (a signed overflow aborts it) and asked for the counts at the edges: no item, one workgroup
exactly and one item more, the largest launch there is (2^31 - 1 workgroups) and one item more, and INT64_MAX items -- where
``(items + per - 1) / per`` would overflow."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "host", "launch_blocks_check.cpp")
MOST = 2 ** 31 - 1  # workgroups of the largest launch
INT64_MAX = 2 ** 63 - 1


def _compiler():
    for c in (os.environ.get("CXX"), "/opt/rocm/lib/llvm/bin/clang++", "clang++", "g++", "c++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = _compiler()
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp("launch_blocks") / "launch_blocks_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True)
    return exe


def _count(checker, items, per):
    """(count, accepted) as the program prints them; a sanitizer report fails the test"""
    p = subprocess.run([checker, str(items), str(per)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and not p.stderr, f"launch_blocks_check {items} {per} failed ({p.returncode}):\n{p.stderr[-2000:]}"
    count, verdict = p.stdout.split()
    assert verdict in ("ok", "refused")
    return int(count), verdict == "ok"


@pytest.mark.parametrize("per", [64, 256])
def test_small_counts(checker, per):
    assert _count(checker, 0, per) == (0, True)  # no item, no workgroup
    assert _count(checker, 1, per) == (1, True)
    assert _count(checker, per, per) == (1, True)
    assert _count(checker, per + 1, per) == (2, True)


@pytest.mark.parametrize("per", [64, 256])
def test_largest_launch_and_beyond(checker, per):
    assert _count(checker, MOST * per, per) == (MOST, True)
    assert _count(checker, MOST * per + 1, per) == (MOST + 1, False)
    count, ok = _count(checker, INT64_MAX, per)  # (items + per - 1 would overflow: the sanitizer would abort the program)
    assert not ok and count == -(-INT64_MAX // per)


def test_a_launcher_refuses_by_name_and_count():
    """launch_blocks through the C ABI: lp_hash_randn (256 numbers per workgroup) refuses 2^31 workgroups before anything is launched
    -- the buffers are never dereferenced -- with LP_EUNSUPPORTED, the entry point's name and the count."""
    from lightplane_amd import _lib
    L = _lib.lib()
    assert L.lp_hash_randn(0x1000, 0x1000, 0x1000, (MOST + 1) * 256, 0, None) == -2
    msg = L.lp_last_error()
    assert b"lp_hash_randn" in msg and str(MOST + 1).encode() in msg

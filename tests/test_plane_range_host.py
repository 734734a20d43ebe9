"""The per-wave sample ranges of the tuned Renderer kernels (csrc/lp_plane_range.h), checked on the CPU.

tests/host/plane_range_check.cpp is a stand-alone program around the very function the kernels call.  It is built here with the
address and undefined-behaviour sanitizers and run over the rays of the headline workload (cfg2: 256 x 256 pinhole rays, axis-aligned
view) and of a 45 deg / 30 deg view: every sample's tap weights are evaluated by brute force, and no sample outside a reported range
may carry a tap of non-zero weight -- zero exceptions.  The fraction of (wave, sample, plane) triples the ranges leave out is printed
(DESIGN.md 4.2 quotes the cfg2 figure)."""
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests.synth import pinhole_rays

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "host", "plane_range_check.cpp")


def _compiler():
    for c in (os.environ.get("CXX"), "/opt/rocm/lib/llvm/bin/clang++", "clang++", "g++", "c++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = _compiler()
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp("plane_range") / "plane_range_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True)
    return exe


def _write_rays(path, rays, S, W, H, D):
    with open(path, "wb") as f:
        f.write(struct.pack("<5i", rays.n_rays, S, W, H, D))
        for t in (rays.origins, rays.directions, rays.near, rays.far):
            f.write(np.ascontiguousarray(t.numpy(), dtype="<f4").tobytes())


def _run(checker, tmp_path, rays, S, W, H, D):
    path = str(tmp_path / "rays.bin")
    _write_rays(path, rays, S, W, H, D)
    p = subprocess.run([checker, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, f"plane_range_check failed ({p.returncode}):\n{p.stderr[-2000:]}"
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert res["violations"] == 0
    return res


def test_cfg2_ranges_are_sound(checker, tmp_path):
    """cfg2 (bench.py): 65 536 rays, S = 128, triplane 64^2.  Geometry: camera at 2.7, near / far bracket the bounding sphere, so the
    samples before and behind the cube miss the xz / yz planes -- at least a quarter of all (wave, sample, plane) triples."""
    res = _run(checker, tmp_path, pinhole_rays(256, 256), 128, 64, 64, 64)
    print("cfg2 plane ranges:", res)
    assert res["triplane_skipped"] <= res["triplane_empty"]  # (the ranges never leave out more than is empty)
    assert res["triplane_skipped"] >= 0.25


def test_elevated_view_ranges_are_sound(checker, tmp_path):
    """45 deg azimuth, 30 deg elevation (the ring cameras of cfg4 / 1080p_s128), a coarser image; S = 128 and an uneven grid."""
    res = _run(checker, tmp_path, pinhole_rays(96, 128, azimuth_deg=45.0, elevation_deg=30.0), 128, 64, 48, 32)
    print("45/30 view plane ranges:", res)
    assert res["triplane_skipped"] <= res["triplane_empty"]


def test_edge_case_batch_ranges_are_sound(checker, tmp_path):
    """The 256 rays of tests/test_gpu_plane_ranges.py (axis-parallel rays, rays grazing a slab face, a lone ray inside a plane for one
    sample, per-ray near / far), S = 32 on 8 cells per axis: the same zero-exceptions check, and the ranges do leave samples out."""
    import torch

    from tests.test_gpu_plane_ranges import G, S, edge_case_rays
    res = _run(checker, tmp_path, edge_case_rays(32, torch.Generator().manual_seed(0)), S, G, G, G)
    print("edge-case batch plane ranges:", res)
    assert res["triplane_skipped"] > 0.2 and res["voxel_skipped"] > 0.2

"""examples/fit_synthetic_scene.py --export-pointcloud: the fitted scene leaves as xyz | rgb | opacity rows of its occupied lattice
points, evaluated by the fused point decoder."""
import importlib.util
import math
import os

import numpy as np
import pytest

import lightplane_amd as lp

pytestmark = pytest.mark.gpu


def test_fit_synthetic_scene_exports_a_pointcloud(tmp_path):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("fit_synthetic_scene", os.path.join(repo, "examples", "fit_synthetic_scene.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    path = str(tmp_path / "cloud.npy")
    size, threshold = 24, 0.05
    old = lp.config.stop_transmittance
    try:
        r = mod.main(["--steps", "30", "--rays", "2048", "--res", "16", "--scaffold-size", str(size), "--scaffold-threshold", str(threshold),
                      "--export-pointcloud", path])
    finally:
        lp.config.stop_transmittance = old
    print("fit with a point cloud:", r)
    assert math.isfinite(r["last_loss"]) and r["pointcloud_file"] == path
    assert "scaffold_steps" not in r  # (the export builds its own scaffold: the fit ran without one)
    cloud = np.load(path)
    assert cloud.dtype == np.float32 and cloud.ndim == 2 and cloud.shape == (r["pointcloud_points"], 7)
    print(f"point cloud: {cloud.shape[0]} of {size ** 3} lattice points, opacity {cloud[:, 6].min():.4g} .. {cloud[:, 6].max():.4g}")
    assert 0 < cloud.shape[0] <= size ** 3
    assert np.isfinite(cloud).all()
    xyz, rgb, opacity = cloud[:, :3], cloud[:, 3:6], cloud[:, 6]
    assert np.abs(xyz).max() <= 1.0 and len(np.unique(xyz, axis=0)) == len(xyz)
    assert rgb.min() >= 0.0 and rgb.max() <= 1.0
    assert (opacity >= 0.0).all() and (opacity > 0.999 * threshold).all()  # (every exported point is an occupied one)

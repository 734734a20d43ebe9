#!/usr/bin/env python
"""Golden files of the reference's ``grid_up_sample`` (examples/utils/util/grid_util.py of a reference checkout; CPU only).

    python tests/golden/make_resample_golden.py <path to the reference checkout>      (or LIGHTPLANE_REFERENCE=<path>)

The helper is imported by path, at generation time only; no reference source is copied, only the numbers it produced.  Every
``gridop_upsample_<case>.npz`` holds the seeded input grids ``in_<k>``, the reference's outputs ``out_<k>``, ``factor`` and
``align_corners`` -- a few KB each.  tests/test_gpu_grid_resample.py holds ``lightplane_amd.grid_up_sample`` to them.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

CASES = {
    "voxel": [(1, 6, 5, 4, 8)],
    "triplane": [(1, 1, 5, 4, 8), (1, 6, 1, 4, 8), (1, 6, 5, 1, 8)],
}
FACTORS = (2.0, 1.5)


def case_names():
    return [f"{kind}_f{str(f).replace('.', 'p')}_{'ac' if ac else 'nac'}" for kind in CASES for f in FACTORS for ac in (False, True)]


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LIGHTPLANE_REFERENCE")
    assert ref, __doc__
    spec = importlib.util.spec_from_file_location("ref_grid_util", os.path.join(ref, "examples", "utils", "util", "grid_util.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    seed = 0
    for kind, shapes in CASES.items():
        for f in FACTORS:
            for ac in (False, True):
                seed += 1
                gen = torch.Generator().manual_seed(seed)
                ins = [torch.randn(*s, generator=gen) for s in shapes]
                outs = mod.grid_up_sample([g.clone() for g in ins], upsample_factor=f, align_corners=ac)
                data = {"factor": np.float64(f), "align_corners": np.int32(ac)}
                for k, (a, b) in enumerate(zip(ins, outs)):
                    data[f"in_{k}"] = a.numpy()
                    data[f"out_{k}"] = b.detach().numpy()
                name = f"gridop_upsample_{kind}_f{str(f).replace('.', 'p')}_{'ac' if ac else 'nac'}.npz"
                np.savez_compressed(os.path.join(HERE, name), **data)
                print(name, [tuple(b.shape) for b in outs])


if __name__ == "__main__":
    main()

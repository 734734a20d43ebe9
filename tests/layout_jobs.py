"""The layout jobs of tests/test_gpu_layouts.py: ``Job``, and one job per front-end of the modular march and of the point ops (the
Renderer / Splatter / embedding / TV jobs stay in the test file).  Inputs and oracles are the ops' own ``tests/*_cases.py``: nothing
here defines an operation a second time -- a job calls the case file's definition on the tensors it is handed.
"""
import torch

import lightplane_amd as lp
from oracle import lightplane_oracle as O
from tests import compositing_cases as CC
from tests import importance_cases as IC
from tests import point_grid_cases as GC
from tests import points_cases as PC
from tests import ray_clip_cases as RC
from tests import ray_loss_cases as LC
from tests.synth import random_rays
from tests.test_gpu_parity import _assert_close, _rel_err

F64 = torch.float64


class Job:
    """One kernel path.  ``inputs``: name -> (CPU values, strided kind of tests/layouts.py, differentiable, is a grid the front-end may
    copy).  Float inputs are fp32; an integer input joins the variants as tests/layouts.py lays integers out.
    ``run(t)``: the call on the tensors ``t`` (name -> tensor) -> list of outputs; the same code runs the HIP path (fp32 on the GPU) and,
    with ``oracle=True``, the fp64 oracle on the CPU.  An output that does not require a gradient is compared like any other and stays
    out of the backward; a job without a differentiable input has no backward."""
    name = ""
    exact_forward = False       # the forward has no atomics: outputs bit-identical to the baseline
    out_tol = 2e-6              # outputs against the baseline otherwise
    config = {}
    strided_raises = None

    def run(self, t, oracle=False):
        raise NotImplementedError

    def up_mask(self, k):
        """``None``, or the CPU fp32 factor of output ``k``'s upstream gradient: 0 at the points where the case file says the derivative
        is not defined to fp32 accuracy (everything is linear in the upstream gradient per point)."""
        return None

    def keep(self, k):
        """``None``, or the bool mask of the entries of output ``k`` whose VALUE is compared (the case file's left-out points)."""
        return None

    def kept(self, k, x):
        x = x.detach().cpu()
        m = self.keep(k)
        return x if m is None else x * m.reshape(m.shape + (1,) * (x.ndim - m.ndim)).to(x.dtype)

    def meets_oracle(self, nm, outs, want):
        """Every output against the fp64 oracle: the project's 1e-4 of the largest entry."""
        assert len(outs) == len(want), f"{nm}: {len(outs)} outputs, the oracle has {len(want)}"
        for k, (o, w) in enumerate(zip(outs, want)):
            o, w = self.kept(k, o), self.kept(k, w)
            print(f"{nm} out{k}: vs oracle {_rel_err(o, w.numpy()):.3e}")
            _assert_close(f"{nm} out{k}/oracle", o, w.numpy())


# ---- the modular march ----------------------------------------------------------------------------------------------------------

R, S = 130, 65  # two full waves of rays plus two; one chunk of samples plus one


def _rays(t, near=None, far=None, gidx=None):
    """``Rays`` of the job's tensors; a field the op does not look at is zeros"""
    d = t["directions"]
    n = d.shape[0]
    zeros = torch.zeros(n, device=d.device, dtype=d.dtype)
    return lp.Rays(directions=d, origins=t["origins"], grid_idx=torch.zeros(n, dtype=torch.long, device=d.device) if gidx is None else gidx,
                   near=zeros if near is None else near, far=zeros if far is None else far, encoding=None)


class RaySamplesJob(Job):
    exact_forward = True
    name = "ray_samples/(9, 3)"

    def __init__(self):
        r = random_rays(torch.Generator().manual_seed(41), R, 2, None)
        self.inputs = {f: (getattr(r, f), "rows", True, False) for f in ("origins", "directions", "near", "far")}

    def run(self, t, oracle=False):
        rays = _rays(t, t["near"], t["far"])
        if oracle:
            return list(CC.placement(rays, 9, 3, 1e-5, F64))
        return list(lp.ray_samples(rays, 9, 3))


class CompositeJob(Job):
    exact_forward = True
    name = "composite/130x65x32 mixed"

    def __init__(self):
        c = CC.inputs(R, S, 32, "mixed")
        self.inputs = {"opacity": (c["opacity"], "rows", True, False), "features": (c["features"], "rows", True, False),
                       "depths": (c["depths"], "columns", True, False), "deltas": (c["deltas"], "rows", True, False)}

    def run(self, t, oracle=False):
        args = (t["opacity"], t["features"], t["depths"], t["deltas"])
        return list(CC.composite(*args)) if oracle else list(lp.composite_samples(*args, return_weights=True))


class ImportanceJob(Job):
    """Regime "transparent": every bin holds mass of the same order, so the inverse CDF's slope is bounded and 1e-4 of the largest
    entry is a bar the new depths can be held to (tests/importance_cases.py on the regimes where it is not)."""
    exact_forward = True
    name = "importance/130x65+63 transparent"
    N = 63

    def __init__(self):
        c = IC.inputs(R, S, self.N, "transparent")
        self.inputs = {"origins": (c["origins"], "rows", True, False), "directions": (c["directions"], "rows", True, False),
                       "depths": (c["depths"], "columns", False, False), "weights": (c["weights"], "rows", False, False),
                       "jitter": (c["jitter"], "columns", False, False)}

    def run(self, t, oracle=False):
        if oracle:
            return list(IC.resample(t["origins"], t["directions"], t["depths"], t["weights"], self.N, jitter=t["jitter"]))
        return list(lp.importance_samples(_rays(t), t["depths"], t["weights"], self.N, include_coarse=True, jitter=t["jitter"]))


class DistortionJob(Job):
    exact_forward = True
    name = "distortion/130x65 mixed"

    def __init__(self):
        c = LC.distortion_inputs(R, S, "mixed")
        self.inputs = {"weights": (c["weights"], "rows", True, False), "depths": (c["depths"], "columns", True, False),
                       "deltas": (c["deltas"], "rows", True, False)}

    def run(self, t, oracle=False):
        args = (t["weights"], t["depths"], t["deltas"])
        return [LC.distortion_pairs(*args) if oracle else lp.distortion_loss(*args)]


class InterlevelJob(Job):
    exact_forward = True
    name = "interlevel/130x65|64 violating"

    def __init__(self):
        c = LC.interlevel_inputs(R, S, 64, "violating")
        self.inputs = {"proposal_weights": (c["proposal_weights"], "rows", True, False), "weights": (c["weights"], "rows", False, False),
                       "depths": (c["depths"], "columns", False, False), "proposal_depths": (c["proposal_depths"], "columns", False, False)}

    def run(self, t, oracle=False):
        if oracle:  # (the definition compares the cells' fp32 edges: the depths go in as the fp32 numbers they are)
            return [LC.interlevel_def(t["weights"].float(), t["depths"].float(), t["proposal_weights"], t["proposal_depths"].float())[0]]
        return [lp.interlevel_loss(t["weights"], t["depths"], t["proposal_weights"], t["proposal_depths"])]


# ---- gather and splat at points -------------------------------------------------------------------------------------------------


def _grid_inputs(c, grids, kind, diff, is_grid):
    """the case's grid-list as job inputs in the case's form: ``grid0 ..`` of a list, ``grid`` the flat tensor"""
    if c["form"] == "flat":
        C = grids[0].shape[-1]
        return {"grid": (torch.cat([g.reshape(-1, C) for g in grids]), kind, diff, is_grid)}
    return {f"grid{i}": (g, kind, diff, is_grid) for i, g in enumerate(grids)}


def _grid_arg(c, t, sizes, prefix="grid"):
    """(the ``grid`` argument, ``grid_sizes``) from the job's tensors"""
    if c["form"] == "flat":
        return t[prefix], sizes
    return [t[f"{prefix}{i}"] for i in range(len(sizes))], None


def _grid_list(c, t, sizes, prefix="grid"):
    """the list of [B, D, H, W, C] tensors the oracle takes (views of the flat tensor)"""
    grid, gs = _grid_arg(c, t, sizes, prefix)
    return list(lp.unflatten_grid(grid, gs)) if gs is not None else grid


class GatherJob(Job):
    """``sample_grid_at_points``: an under-aligned grid is cloned with the warning (as the Renderer does), a grid that is not dense is
    refused (test_as_is_inputs_are_refused): the strided variant keeps the grids fresh.  The grid gradient is a splat (atomics)."""
    exact_forward = True

    def __init__(self, case):
        self.name = f"gather/{case}"
        c = self.c = GC.case(case)
        self.inputs = {"points": (c["pts"], "rows", True, False), **_grid_inputs(c, c["grids"], "offset_only", True, True),
                       "gidx": (c["gidx"], "rows", False, False)}

    def up_mask(self, k):
        return (~self.c["zeroed"]).float()[..., None]

    def run(self, t, oracle=False):
        c = self.c
        if oracle:
            q = O.contract_pi(t["points"]) if c["contract"] else t["points"]
            return [O.sample_grid_list(_grid_list(c, t, c["sizes"]), q, t["gidx"], c["mask"])]
        grid, sizes = _grid_arg(c, t, c["sizes"])
        return [lp.sample_grid_at_points(t["points"], grid, t["gidx"], c["mask"], c["contract"], grid_sizes=sizes)]


class SplatJob(Job):
    """``splat_points`` into a list.  The features are the case's ``vec_live`` -- zero where the interpolation weights have a kink --
    so that the raw splat's point gradient is defined at every point (tests/point_grid_cases.py); the oracle is the case file's: the
    adjoint of its bilinear form, and ``F / clamp(W, 1e-5)`` with ``W`` the splat of ones.  Outputs are sums of atomics."""

    def __init__(self, case, normalize):
        self.name = f"splat_{'norm' if normalize else 'raw'}/{case}"
        self.normalize = normalize
        c = self.c = GC.case(case)
        assert c["form"] == "list" and not bool(c["left_out"].any())
        self.inputs = {"points": (c["pts"], "rows", not normalize, False), "features": (c["vec_live"], "rows", True, False),
                       "gidx": (c["gidx"], "rows", False, False)}

    def _adjoint(self, points, vectors, channels):
        c = self.c
        zeros = [torch.zeros(s[:4] + [channels], dtype=F64, requires_grad=True) for s in c["sizes"]]
        form = GC.bilinear_form(zeros, points, c["gidx"], vectors, c["mask"], c["contract"])
        return list(torch.autograd.grad(form, zeros, create_graph=True))

    def run(self, t, oracle=False):
        c = self.c
        if not oracle:
            return list(lp.splat_points(t["points"], t["features"], c["sizes"], t["gidx"], c["mask"], c["contract"], normalize=self.normalize))
        raw = self._adjoint(t["points"], t["features"], c["sizes"][0][4])
        if not self.normalize:
            return raw
        ones = torch.ones(tuple(t["points"].shape[:2]) + (1,), dtype=F64)
        return [f / w.detach().clamp(min=1e-5) for f, w in zip(raw, self._adjoint(t["points"].detach(), ones, 1))]


# ---- the decoder at points ------------------------------------------------------------------------------------------------------


class PointsJob(Job):
    """``lightplane_eval_mlp`` / ``_opacity_only``.  The grids go to the library AS THEY ARE: fresh in every variant, and no warning may
    fire (their refusals: test_as_is_inputs_are_refused).  Left-out and zeroed points are the case's own (tests/points_cases.py).
    The forward has no atomics; the grid and ``mlp_params`` gradients are sums of atomics."""
    exact_forward = True

    def __init__(self, case, opacity_only=False):
        self.name = f"points{'_opacity' if opacity_only else ''}/{case}"
        self.opacity_only = opacity_only
        c = self.c = PC.case(case)
        assert c["cgrids"] is None or not opacity_only
        self.sizes = [list(g.shape) for g in c["grids"]]
        self.inputs = {"points": (c["pts"], "rows", True, False), "mlp_params": (c["dec"].mlp_params, "rows", True, False)}
        if not opacity_only:
            self.inputs["rays_encoding"] = (c["enc"], "columns", True, False)
        self.inputs.update(_grid_inputs(c, c["grids"], "as_is", True, False))
        if c["cgrids"] is not None:
            self.inputs.update({"color_" + n: v for n, v in _grid_inputs(c, c["cgrids"], "as_is", True, False).items()})
        if c["scaffold"] is not None:  # (channels-first and permuted: every other row of a [2, D, H, W] tensor is dense for B = 1)
            self.inputs["scaffold"] = (c["scaffold"], "grid", False, False)
        self.inputs["gidx"] = (c["gidx"], "rows", False, False)

    def up_mask(self, k):
        live = (~self.c["zeroed"]).float()
        return live if k == 0 else live[..., None]

    def keep(self, k):
        return ~self.c["left_out"]

    def run(self, t, oracle=False):
        c = self.c
        d = c["dec"]
        dec = lp.DecoderParams(t["mlp_params"], d.n_hidden_trunk, d.n_hidden_opacity, d.n_hidden_color, d.color_chn)
        sc = t.get("scaffold")
        two = c["cgrids"] is not None
        if oracle:
            enc = c["enc"].double() if self.opacity_only else t["rays_encoding"]
            op, col = O.eval_decoder(t["points"], _grid_list(c, t, self.sizes), t["gidx"], dec, enc, PC.GAIN,
                                     mask_out_of_bounds_samples=c["mask"], scaffold=sc, contract_coords=c["contract"],
                                     color_grids=_grid_list(c, t, self.sizes, "color_grid") if two else None)
            return [op] if self.opacity_only else [op, col[..., :3]]
        grid, sizes = _grid_arg(c, t, self.sizes)
        cgrid, csizes = _grid_arg(c, t, self.sizes, "color_grid") if two else (None, None)
        if self.opacity_only:
            return [lp.lightplane_eval_mlp_opacity_only(t["points"], grid, t["gidx"], dec, PC.GAIN, c["mask"], None, sc, c["contract"],
                                                        grid_sizes=sizes)]
        return list(lp.lightplane_eval_mlp(t["points"], grid, t["gidx"], dec, t["rays_encoding"], PC.GAIN, c["mask"], None, sc, cgrid,
                                           c["contract"], grid_sizes=sizes, color_grid_sizes=csizes))


# ---- the ray clip ---------------------------------------------------------------------------------------------------------------


class RayClipJob(Job):
    """``clip_rays_to_scaffold`` copies an under-aligned ray field or scaffold and refuses one that is not dense.  Nothing is
    differentiable.  The oracle is the brute force of tests/ray_clip_cases.py, computed with the case; a clipped span is held to it by
    the case file's own checks (conservative, exact misses, tight to the derived tolerance) -- 1e-4 of the largest entry is not its bar."""
    exact_forward = True
    strided_raises = "contiguous"
    PAD = 0.5

    def __init__(self, case="random_2x5x6x7"):
        self.name = f"ray_clip/{case}"
        c = self.c = RC.case(case)
        self.inputs = {"directions": (c["d"], "rows", False, False), "origins": (c["o"], "rows", False, False),
                       "near": (c["near"], "rows", False, False), "far": (c["far"], "rows", False, False),
                       "scaffold": (c["scaffold"], "rows", False, False), "gidx": (c["grid_idx"], "rows", False, False)}

    def rays(self, t):
        return _rays(t, t["near"], t["far"], t["gidx"])

    def run(self, t, oracle=False, out=None):
        if oracle:
            return []  # (the case holds its oracle; meets_oracle reads it)
        clipped, hit = lp.clip_rays_to_scaffold(self.rays(t), t["scaffold"], pad=self.PAD, out=out)
        return [clipped.near, clipped.far, hit]

    def meets_oracle(self, nm, outs, want):
        near, far, hit = (o.detach().cpu() for o in outs)
        assert hit.dtype == torch.bool
        RC.check_conservative(self.c, near, far, hit)
        RC.check_misses(self.c, near, far, hit)
        n, worst = RC.check_tight(self.c, near, far, hit, self.PAD)
        print(f"{nm}: {n} rays compared, the loosest end uses {worst:.3f} of its tolerance (2 allowed outwards)")
        assert n > 50


NEW_JOBS = [
    ("ray_samples", RaySamplesJob),
    ("composite", CompositeJob),
    ("importance", ImportanceJob),
    ("distortion", DistortionJob),
    ("interlevel", InterlevelJob),
    ("gather", lambda: GatherJob("triplane_c16")),
    ("gather_flat", lambda: GatherJob("voxel_c32_flat")),
    ("splat_raw", lambda: SplatJob("triplane_c16", False)),
    ("splat_norm", lambda: SplatJob("triplane_c16", True)),
    ("points", lambda: PointsJob("triplane_c16_222x32")),
    ("points_opacity_scaffold", lambda: PointsJob("triplane_c20_222x33_scaffold", opacity_only=True)),
    ("ray_clip", RayClipJob),
]

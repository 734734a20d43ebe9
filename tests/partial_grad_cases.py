"""The launches of the partial-gradient tests: one entry per backward path whose control flow depends on WHICH gradients the
caller asks for (tests/test_partial_grads_host.py checks the table without a GPU, tests/test_gpu_partial_grads.py runs it).

The C ABI (include/lightplane_hip.h) says of a backward's result buffers "NULL = skip" and of its upstream gradients
"NULL = zeros"; the front-ends pass NULL for every leaf that does not require a gradient.  The kernels turn those NULLs into
other control flow -- ``want_params`` removes the workgroup barriers and the X / dY tile stores of the tuned family's sample loop,
``gg`` / ``ggs`` trunk layer 1's dX product and the scatter, ``ggc`` the colour-grid scatter between two layer phases of the looped
family, ``lds_acc`` the LDS layout of the shape-generic launches -- so every entry names the path it is meant to reach, the switches
that reach it and the selection the library's own host queries have to report for it.

Shapes: 160 rays (MFMA families: one full four-wave workgroup of 128 rays + a tail workgroup with one wave of rays and three of
invalid lanes only; shape-generic kernels: two full 64-ray blocks and a half-filled one), grids of the sizes of tests/synth.py (4 to
8 cells per axis), 21 samples where the segmented march is meant (three LP_SEG_LEN blocks, the last one partial), 33 where the
transposed march is meant (it needs 32).  Every entry that is not about the segmented march switches it off
(``config.segment_forward = segment_backward = False``): a batch this small would take it by default.
"""
from __future__ import annotations

import contextlib
import dataclasses
import itertools
from dataclasses import dataclass, field
from typing import Tuple

import lightplane_amd as lp
from lightplane_amd import _lib
from tests.synth import RENDERER_CASES, SPLATTER_CASES, RendererCase, SplatterCase

N_RAYS = 160
NO_SEG = dict(segment_forward=False, segment_backward=False)


def _r(name, **kw) -> RendererCase:
    return dataclasses.replace(next(c for c in RENDERER_CASES if c.name == name), n_rays=N_RAYS, **kw)


def _s(name, **kw) -> SplatterCase:
    return dataclasses.replace(next(c for c in SPLATTER_CASES if c.name == name), n_rays=N_RAYS, **kw)


@contextlib.contextmanager
def config_set(**kw):
    """``lightplane_amd.config`` attributes for the duration of the block, restored in ``finally``."""
    old = {k: getattr(lp.config, k) for k in kw}
    for k, v in kw.items():
        setattr(lp.config, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(lp.config, k, v)


@dataclass(frozen=True)
class RendererEntry:
    id: str
    path: str                      # the backward path the entry is meant to reach
    case: RendererCase
    # the switches that reach it
    config: dict = field(default_factory=lambda: dict(NO_SEG))
    kernel: int = _lib.LP_KERNEL_AUTO
    march_order: str = "rays"
    flat: bool = False             # one flat [rows, C] grid tensor + grid_sizes instead of the list
    # the selection the host queries have to report
    family: int = 1
    segments: int = 1
    extra_subsets: Tuple[Tuple[str, ...], ...] = ()

    @property
    def two_grid(self) -> bool:
        return self.case.separate_color_grid

    @property
    def arithmetic(self) -> int:
        return int(self.config.get("arithmetic", _lib.LP_ARITH_DEFAULT))

    @property
    def segmented(self) -> bool:
        return self.segments > 1

    @property
    def encoding_is_written(self) -> bool:
        """LpRendererArgs.grad_encoding is "written, not accumulated" by a one-sweep backward; the segments of a segmented one
        accumulate it."""
        return self.segments == 1

    def call_kwargs(self) -> dict:
        return dict(kernel=self.kernel, march_order=self.march_order)

    def subsets(self):
        return renderer_subsets(self)


@dataclass(frozen=True)
class SplatterEntry:
    id: str
    path: str
    case: SplatterCase
    kernel: int = _lib.LP_KERNEL_AUTO
    family: int = 3
    segments: int = 1
    blocks: int = 1                # 32-unit blocks per layer of the looped family (0: shape-generic)

    @property
    def encoding_is_written(self) -> bool:
        return self.segments == 1

    def subsets(self):
        return SPLATTER_SUBSETS


_GENERIC_GLOBAL = RendererCase("generic_global", seed=41, n_rays=N_RAYS, is_triplane=True, hidden=64, n_layers=(3, 3, 3), param_std=0.1)

RENDERER_ENTRIES = [
    RendererEntry("tuned_tri_c16", "tuned four-wave full-batch kernel, plain march, triplane, 16 channels", _r("triplane_basic"),
                  extra_subsets=(("G1",),)),
    RendererEntry("tuned_vox_c32", "tuned four-wave full-batch kernel, plain march, voxel grid, 32 channels",
                  _r("voxel_basic", seed=42, grid_base=(2, 6, 5, 7, 32))),
    RendererEntry("tuned_nonplain", "tuned full-batch kernel, non-plain instantiation (contraction, beyond-far samples, noise)",
                  _r("triplane_basic", seed=43, contract=True, num_samples_inf=3, noise_sigma=0.5, noise_seed=77)),
    RendererEntry("tuned_seg", "segment-parallel tuned backward (grad_encoding accumulated over the segments)",
                  _r("triplane_basic", seed=44, num_samples=21), config={}, segments=3),
    RendererEntry("tuned_nw8", "tuned family, eight-wave workgroups (more than 64 beyond-far samples)",
                  _r("voxel_basic", seed=45, num_samples=11, num_samples_inf=70, gain=0.25, contract=True)),
    RendererEntry("tuned_tm", "tuned family, transposed march (32 samples of a ray per wavefront)",
                  _r("triplane_basic", seed=46, num_samples=33), march_order="samples"),
    RendererEntry("tuned_fp32", "tuned family, LP_ARITH_FP32: the fp32 dW form (no DWB) and three-limb dX chains",
                  _r("triplane_basic", seed=47), config=dict(NO_SEG, arithmetic=_lib.LP_ARITH_FP32)),
    RendererEntry("loop_deep_424", "layer-looped family, deep instantiation", _r("voxel_deep"), family=3),
    RendererEntry("loop_shallow_h16", "layer-looped family, shallow instantiation (1/1/1 x 16)", _r("nb1_like_h16_111"), family=3),
    RendererEntry("loop_h64_two_block", "layer-looped two-block kernels (hidden 64): z_delta path of loop_layer_bwd",
                  _r("triplane_h64_c32"), family=3),
    RendererEntry("loop_c64", "layer-looped two-block kernels (64 grid channels)", _r("triplane_c64_h32"), family=3),
    RendererEntry("loop_seg", "layer-looped family, segment-parallel march", _r("voxel_deep", seed=48, num_samples=21), config={},
                  family=3, segments=3),
    RendererEntry("loop_two_grid", "layer-looped family, separate colour grid-list (TG, ggc)", _r("colorgrid_c32_mixed"), family=3,
                  extra_subsets=(("Cg",), ("G", "Cg"), ("P", "Cg"))),
    RendererEntry("loop_two_grid_h64", "layer-looped two-block kernels, separate colour grid-list", _r("colorgrid_h64_c32_triplane"),
                  family=3, extra_subsets=(("Cg",), ("G", "Cg"), ("P", "Cg"))),
    RendererEntry("generic_lds", "shape-generic backward, parameter gradients accumulated in LDS (lds_acc)", _r("triplane_basic", seed=49),
                  kernel=_lib.LP_KERNEL_GENERIC, family=0),
    RendererEntry("generic_global", "shape-generic backward, parameters beyond the 96 KB of lds_acc: global atomics", _GENERIC_GLOBAL,
                  kernel=_lib.LP_KERNEL_GENERIC, family=0),
    RendererEntry("flat_grid", "flat [rows, C] grid tensor + grid_sizes (LpRendererArgs.grad_grid, not the per-grid list)",
                  _r("triplane_plus_voxel"), flat=True),
]

SPLATTER_ENTRIES = [
    SplatterEntry("mlp_loop_h32", "MLP-Splatter, layer-looped family, hidden 32", _s("mlp2_voxel")),
    SplatterEntry("mlp_loop_two_block", "MLP-Splatter, layer-looped two-block kernels (hidden 64)", _s("mlp3_voxel_h64_f32"), blocks=2),
    SplatterEntry("mlp_loop_seg", "MLP-Splatter, layer-looped family, segmented march (grad_encoding: atomics behind a memset)",
                  _s("mlp2_voxel", seed=50, num_samples=70), segments=4),
    SplatterEntry("mlp_generic", "MLP-Splatter, shape-generic kernels", _s("mlp2_voxel", seed=51), kernel=_lib.LP_KERNEL_GENERIC, family=0,
                  blocks=0),
]

# ---- leaf subsets ----------------------------------------------------------------------------------------------------------
# Renderer leaves: P = mlp_params, E = rays.encoding, G = every grid tensor, Cg = every colour-grid tensor (two-grid entries),
# G1 = the second tensor of a grid list alone (the front-end allocates all buffers and hands back one).
RENDERER_BASE_SUBSETS = (("P",), ("E",), ("G",), ("P", "E"), ("P", "G"), ("E", "G"))
TWO_GRID_SUBSETS = (("Cg",), ("G", "Cg"), ("P", "Cg"))
SPLATTER_LEAVES = ("E", "P", "G")   # encoding, mlp_params, input grids
SPLATTER_SUBSETS = tuple(s for k in (1, 2) for s in itertools.combinations(SPLATTER_LEAVES, k))


def renderer_subsets(e: RendererEntry):
    return RENDERER_BASE_SUBSETS + e.extra_subsets


# ---- upstream gradients left out ("NULL = zeros") ---------------------------------------------------------------------------
NULL_UPSTREAM_ENTRIES = ("tuned_tri_c16", "tuned_seg", "tuned_tm", "tuned_nw8", "loop_deep_424", "loop_two_grid", "generic_lds")
# which of (g_len, g_nlt, g_feat) are GIVEN; the others reach the kernels as NULL pointers
NULL_UPSTREAM_PATTERNS = {"len": (True, False, False), "feature": (False, False, True), "nlt": (False, True, False),
                          "len+feature": (True, False, True)}


def subset_id(s) -> str:
    return "+".join(s)


def renderer_entry(entry_id: str) -> RendererEntry:
    return next(e for e in RENDERER_ENTRIES if e.id == entry_id)


# ---- what the library's own host queries say (no GPU needed) ------------------------------------------------------------------
def renderer_selection(e: RendererEntry, d=None) -> dict:
    """Kernel family, backward segments and march order of the entry's call, from ``lp.kernel_family`` / ``lp.backward_segments``
    under the entry's ``config``.  The front-end asks for segment records only with ``config.segment_backward`` on
    (LightplaneFunction.forward); without them every family sweeps a ray once, whatever ``lp_renderer_backward_segments`` offers."""
    d = e.case.build() if d is None else d
    cfg = d["cfg"]
    with config_set(**e.config):
        fam = lp.kernel_family(d["rays"], d["grids"], d["decoder"], color_grid=d["color_grids"], num_samples_inf=cfg["num_samples_inf"],
                               kernel=e.kernel)
        offered = lp.backward_segments(d["rays"], d["grids"], d["decoder"], cfg["num_samples"], cfg["num_samples_inf"],
                                       color_grid=d["color_grids"], kernel=e.kernel, march_order=e.march_order)
        segments = offered if lp.config.segment_backward else 1
    transposed = (fam == 1 and e.march_order == "samples" and cfg["num_samples"] >= 32 and cfg["num_samples_inf"] == 0
                  and e.arithmetic == _lib.LP_ARITH_DEFAULT)
    return dict(family=fam, segments=segments, offered_segments=offered, march="samples" if transposed else "rays")


def splatter_selection(e: SplatterEntry, d=None) -> dict:
    from lightplane_amd.splatter import mlp_splatter_kernel_family, mlp_splatter_launch_shape
    d = e.case.build() if d is None else d
    cfg = d["cfg"]
    shape = mlp_splatter_launch_shape(e.case.n_rays, d["out_sizes"], d["mlp"], d["in_sizes"], cfg["num_samples"], cfg["num_samples_inf"],
                                      kernel=e.kernel)
    native = mlp_splatter_kernel_family(d["out_sizes"], d["mlp"], d["in_sizes"], cfg["num_samples_inf"])
    return dict(family=shape["family"], native_family=native, segments=shape["bwd_segments"], blocks=shape["blocks"])

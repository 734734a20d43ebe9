"""ctypes binding of ``liblightplane_hip.so`` (C ABI: ``include/lightplane_hip.h``).

The structures below mirror the header field for field.  There is NO fallback: if
the shared library is missing, ``lib()`` raises -- build it with
``python lightplane_amd/csrc/build.py`` (or ``__graft_entry__.build()``).
"""
from __future__ import annotations

import ctypes as C
import os
import warnings
from typing import Optional, Sequence

import torch

from .params import mlp_numel

LP_MAX_GRIDS = 8
LP_MAX_LAYERS = 8
LP_MAX_WIDTH = 128
LP_NLT_CKPT = 32
LP_SEG_LEN = 8   # samples per state record of a small batch's segment-parallel march (lightplane_hip.h; 16 before ABI 0.2.7)


def n_nlt_ckpt(num_samples: int, num_samples_inf: int) -> int:
    """Floats per ray of the -log T checkpoint buffer: one (hi, lo) float pair per checkpoint plus the
    closing pair (see LP_NLT_CKPT in the header)."""
    c = LP_NLT_CKPT
    return 2 * ((num_samples + c - 1) // c + num_samples_inf + 1)

LP_KERNEL_AUTO, LP_KERNEL_GENERIC, LP_KERNEL_MFMA = 0, 1, 2
LP_ARITH_DEFAULT, LP_ARITH_FP32 = 0, 1  # LpRendererArgs.arithmetic (include/lightplane_hip.h)
LP_MARCH_RAYS_PER_WAVE, LP_MARCH_SAMPLES_PER_WAVE = 0, 1  # LpRendererArgs.march_order

_f32p = C.POINTER(C.c_float)
_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)


class LpGrid(C.Structure):
    _fields_ = [("B", C.c_int32), ("D", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("row_offset", C.c_int64), ("data", C.c_void_p)]


class LpGridList(C.Structure):
    _fields_ = [("data", C.c_void_p), ("n_grids", C.c_int32), ("channels", C.c_int32),
                ("n_rows", C.c_int64), ("grids", LpGrid * LP_MAX_GRIDS)]


class LpRays(C.Structure):
    _fields_ = [("n_rays", C.c_int64), ("directions", C.c_void_p), ("origins", C.c_void_p),
                ("grid_idx", C.c_void_p), ("near_t", C.c_void_p), ("far_t", C.c_void_p),
                ("encoding", C.c_void_p), ("encoding_dim", C.c_int32), ("row_length", C.c_int32)]


class LpMarch(C.Structure):
    _fields_ = [("num_samples", C.c_int32), ("num_samples_inf", C.c_int32),
                ("mask_out_of_bounds", C.c_int32), ("contract_coords", C.c_int32),
                ("disparity_at_inf", C.c_double)]


class LpMlp(C.Structure):
    _fields_ = [("n_layers", C.c_int32), ("dims", C.c_int32 * (LP_MAX_LAYERS + 1)),
                ("offset", C.c_int64)]


class LpRendererArgs(C.Structure):
    _fields_ = [
        ("rays", LpRays), ("grid", LpGridList), ("color_grid", LpGridList),
        ("scaffold", C.c_void_p), ("scaffold_shape", LpGrid), ("march", LpMarch),
        ("mlp_params", C.c_void_p), ("n_mlp_params", C.c_int64),
        ("trunk", LpMlp), ("opacity", LpMlp), ("color", LpMlp),
        ("color_chn", C.c_int32), ("gain", C.c_float), ("noise_sigma", C.c_float),
        ("noise_seed", C.c_int32), ("kernel", C.c_int32), ("seg_forward_off", C.c_int32),
        ("ray_length", C.c_void_p), ("neg_log_t", C.c_void_p), ("feature", C.c_void_p),
        ("neg_log_t_ckpt", C.c_void_p),
        ("grad_ray_length", C.c_void_p), ("grad_neg_log_t", C.c_void_p), ("grad_feature", C.c_void_p),
        ("grad_grid", C.c_void_p), ("grad_color_grid", C.c_void_p), ("grad_mlp_params", C.c_void_p),
        ("grad_encoding", C.c_void_p),
        ("grad_grid_list", C.c_void_p * LP_MAX_GRIDS), ("grad_color_grid_list", C.c_void_p * LP_MAX_GRIDS),
        ("bg_color", C.c_void_p), ("alpha", C.c_void_p), ("grad_alpha", C.c_void_p), ("alpha_mode", C.c_int32),
        ("stop_neg_log_t", C.c_float), ("seg_prefix", C.c_void_p), ("arithmetic", C.c_int32), ("march_order", C.c_int32),
    ]


class LpSplatterArgs(C.Structure):
    _fields_ = [
        ("rays", LpRays), ("march", LpMarch), ("out", LpGridList),
        ("out_feature", C.c_void_p), ("out_weight", C.c_void_p),
        ("input_grid", LpGridList), ("mlp_params", C.c_void_p), ("n_mlp_params", C.c_int64),
        ("mlp", LpMlp), ("kernel", C.c_int32), ("march_order", C.c_int32),
        ("grad_out", C.c_void_p), ("weight", C.c_void_p), ("grad_encoding", C.c_void_p),
        ("grad_input_grid", C.c_void_p), ("grad_mlp_params", C.c_void_p),
        ("grad_input_grid_list", C.c_void_p * LP_MAX_GRIDS),
    ]


class LpRayEmbedArgs(C.Structure):
    _fields_ = [
        ("n_rays", C.c_int64), ("directions", C.c_void_p), ("n_harmonics", C.c_int32), ("out_dim", C.c_int32),
        ("weight", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p), ("grad_out", C.c_void_p),
        ("grad_weight", C.c_void_p), ("grad_bias", C.c_void_p),
    ]


class LpScaffoldArgs(C.Structure):
    _fields_ = [
        ("grid", LpGridList), ("mlp_params", C.c_void_p), ("n_mlp_params", C.c_int64),
        ("trunk", LpMlp), ("opacity", LpMlp), ("gain", C.c_float), ("mask_out_of_bounds", C.c_int32),
        ("shape", LpGrid), ("threshold", C.c_float), ("dilate", C.c_int32),
    ]


class LpPointsArgs(C.Structure):
    _fields_ = [
        ("grid", LpGridList), ("color_grid", LpGridList), ("mlp_params", C.c_void_p), ("n_mlp_params", C.c_int64),
        ("trunk", LpMlp), ("opacity", LpMlp), ("color", LpMlp),
        ("color_chn", C.c_int32), ("gain", C.c_float), ("mask_out_of_bounds", C.c_int32), ("contract_coords", C.c_int32),
        ("points", C.c_void_p), ("grid_idx", C.c_void_p), ("encoding", C.c_void_p), ("encoding_dim", C.c_int32), ("reserved", C.c_int32),
        ("n_rays", C.c_int64), ("n_pts", C.c_int64), ("scaffold", C.c_void_p), ("scaffold_shape", LpGrid),
        ("opacity_out", C.c_void_p), ("color_out", C.c_void_p), ("grad_opacity", C.c_void_p), ("grad_color", C.c_void_p),
        ("grad_grid", C.c_void_p), ("grad_color_grid", C.c_void_p),
        ("grad_grid_list", C.c_void_p * LP_MAX_GRIDS), ("grad_color_grid_list", C.c_void_p * LP_MAX_GRIDS),
        ("grad_mlp_params", C.c_void_p), ("grad_encoding", C.c_void_p), ("grad_points", C.c_void_p),
    ]


class LpRayClipArgs(C.Structure):
    _fields_ = [("rays", LpRays), ("scaffold", C.c_void_p), ("scaffold_shape", LpGrid), ("pad", C.c_float), ("reserved", C.c_int32)]


class LpPointGridArgs(C.Structure):
    _fields_ = [
        ("grid", LpGridList), ("row_weight", C.c_void_p * LP_MAX_GRIDS), ("points", C.c_void_p), ("grid_idx", C.c_void_p),
        ("n_rays", C.c_int64), ("n_pts", C.c_int64), ("vectors", C.c_void_p), ("out_features", C.c_void_p), ("grad_points", C.c_void_p),
        ("channels", C.c_int32), ("mask_out_of_bounds", C.c_int32), ("contract_coords", C.c_int32), ("reserved", C.c_int32),
    ]


class LpMeshArgs(C.Structure):
    _fields_ = [
        ("volume", C.c_void_p), ("shape", LpGrid), ("level", C.c_float), ("reserved", C.c_int32),
        ("vertex_offsets", C.c_void_p), ("face_offsets", C.c_void_p), ("vertices", C.c_void_p), ("faces", C.c_void_p),
        ("normals", C.c_void_p), ("max_vertices", C.c_int64), ("max_faces", C.c_int64),
    ]


class LpRaySamplesArgs(C.Structure):  # include/lightplane_hip_samples.h
    _fields_ = [
        ("rays", LpRays), ("march", LpMarch), ("points", C.c_void_p), ("depths", C.c_void_p), ("deltas", C.c_void_p),
        ("grad_points", C.c_void_p), ("grad_depths", C.c_void_p), ("grad_deltas", C.c_void_p),
        ("grad_origins", C.c_void_p), ("grad_directions", C.c_void_p), ("grad_near", C.c_void_p), ("grad_far", C.c_void_p),
    ]


class LpCompositeArgs(C.Structure):  # include/lightplane_hip_samples.h
    _fields_ = [
        ("opacity", C.c_void_p), ("features", C.c_void_p), ("depths", C.c_void_p), ("deltas", C.c_void_p),
        ("n_rays", C.c_int64), ("n_samples", C.c_int32), ("channels", C.c_int32),
        ("ray_length", C.c_void_p), ("neg_log_t", C.c_void_p), ("feature", C.c_void_p), ("weights", C.c_void_p),
        ("grad_ray_length", C.c_void_p), ("grad_neg_log_t", C.c_void_p), ("grad_feature", C.c_void_p), ("grad_weights", C.c_void_p),
        ("grad_opacity", C.c_void_p), ("grad_features", C.c_void_p), ("grad_depths", C.c_void_p), ("grad_deltas", C.c_void_p),
    ]


class LpImportanceArgs(C.Structure):  # include/lightplane_hip_importance.h
    _fields_ = [
        ("origins", C.c_void_p), ("directions", C.c_void_p), ("depths", C.c_void_p), ("weights", C.c_void_p), ("jitter", C.c_void_p),
        ("n_rays", C.c_int64), ("n_samples", C.c_int32), ("n_importance", C.c_int32), ("include_coarse", C.c_int32), ("pad", C.c_float),
        ("out_points", C.c_void_p), ("out_depths", C.c_void_p), ("out_deltas", C.c_void_p),
        ("grad_points", C.c_void_p), ("grad_origins", C.c_void_p), ("grad_directions", C.c_void_p),
    ]


class LpDistortionArgs(C.Structure):  # include/lightplane_hip_losses.h
    _fields_ = [
        ("weights", C.c_void_p), ("depths", C.c_void_p), ("deltas", C.c_void_p), ("grad_loss", C.c_void_p), ("loss", C.c_void_p),
        ("grad_weights", C.c_void_p), ("grad_depths", C.c_void_p), ("grad_deltas", C.c_void_p),
        ("n_rays", C.c_int64), ("n_samples", C.c_int32), ("reserved", C.c_int32),
    ]


class LpInterlevelArgs(C.Structure):  # include/lightplane_hip_losses.h
    _fields_ = [
        ("weights", C.c_void_p), ("depths", C.c_void_p), ("proposal_weights", C.c_void_p), ("proposal_depths", C.c_void_p),
        ("grad_loss", C.c_void_p), ("loss", C.c_void_p), ("grad_proposal_weights", C.c_void_p),
        ("n_rays", C.c_int64), ("n_samples", C.c_int32), ("n_proposal", C.c_int32), ("eps", C.c_float), ("reserved", C.c_int32),
    ]


class LpRenderSamplesArgs(C.Structure):  # include/lightplane_hip_render_samples.h
    _fields_ = [
        ("grid", LpGridList), ("color_grid", LpGridList), ("mlp_params", C.c_void_p), ("n_mlp_params", C.c_int64),
        ("trunk", LpMlp), ("opacity", LpMlp), ("color", LpMlp),
        ("color_chn", C.c_int32), ("gain", C.c_float), ("mask_out_of_bounds", C.c_int32), ("contract_coords", C.c_int32),
        ("origins", C.c_void_p), ("directions", C.c_void_p), ("grid_idx", C.c_void_p), ("encoding", C.c_void_p),
        ("encoding_dim", C.c_int32), ("n_samples", C.c_int32), ("n_rays", C.c_int64), ("depths", C.c_void_p), ("deltas", C.c_void_p),
        ("scaffold", C.c_void_p), ("scaffold_shape", LpGrid),
        ("ray_length", C.c_void_p), ("neg_log_t", C.c_void_p), ("feature", C.c_void_p), ("weights", C.c_void_p), ("chunk_nlt", C.c_void_p),
        ("grad_ray_length", C.c_void_p), ("grad_neg_log_t", C.c_void_p), ("grad_feature", C.c_void_p), ("grad_weights", C.c_void_p),
        ("grad_grid", C.c_void_p), ("grad_color_grid", C.c_void_p),
        ("grad_grid_list", C.c_void_p * LP_MAX_GRIDS), ("grad_color_grid_list", C.c_void_p * LP_MAX_GRIDS),
        ("grad_mlp_params", C.c_void_p), ("grad_encoding", C.c_void_p),
    ]


class LpRayGridArgs(C.Structure):  # include/lightplane_hip_ray_grid.h
    _fields_ = [
        ("grid", LpGridList), ("row_weight", C.c_void_p * LP_MAX_GRIDS),
        ("origins", C.c_void_p), ("directions", C.c_void_p), ("grid_idx", C.c_void_p), ("depths", C.c_void_p), ("weights", C.c_void_p),
        ("vectors", C.c_void_p), ("out_features", C.c_void_p), ("grad_weights", C.c_void_p), ("grad_depths", C.c_void_p),
        ("n_rays", C.c_int64), ("n_samples", C.c_int32), ("channels", C.c_int32),
        ("mask_out_of_bounds", C.c_int32), ("contract_coords", C.c_int32),
    ]


_LIB = None
LIB_PATH = os.environ.get("LIGHTPLANE_AMD_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "liblightplane_hip.so")

#: every symbol include/lightplane_hip.h declares
EXPORTS = (
    "lp_version", "lp_last_error", "lp_abi_sizeof", "lp_renderer_forward", "lp_renderer_backward",
    "lp_splatter_forward", "lp_splatter_normalize", "lp_splatter_backward", "lp_hash_randn",
    "lp_renderer_forward_family", "lp_renderer_forward_ws",  # (+ lp_renderer_forward_workspace_bytes, which returns int64_t)
    "lp_renderer_corner_rows", "lp_renderer_kernel_family", "lp_splatter_kernel_family",
    "lp_renderer_backward_segments", "lp_renderer_backward_relu_dump", "lp_renderer_relu_dump_words", "lp_build_info",
    "lp_ray_embedding_forward", "lp_ray_embedding_backward",
    "lp_mlp_splatter_backward_relu_dump", "lp_mlp_splatter_relu_dump_words", "lp_mlp_splatter_launch_shape",
    "lp_grid_tv_forward", "lp_grid_tv_backward", "lp_grid_tv_fused",  # (+ lp_grid_tv_workspace_bytes, which returns int64_t)
    "lp_grid_resample_forward", "lp_grid_resample_backward",
    "lp_scaffold_opacity", "lp_scaffold_build",  # (+ lp_scaffold_workspace_bytes, which returns int64_t)
    "lp_points_forward", "lp_points_backward",
    "lp_rays_clip",
    "lp_point_gather", "lp_point_splat", "lp_point_normalize", "lp_point_grad_points",
    "lp_mesh_count", "lp_mesh_emit",  # (+ lp_mesh_workspace_bytes, which returns int64_t)
)

#: every symbol include/lightplane_hip_samples.h declares (a header and a table of their own: the ones above stay as they are)
SAMPLES_EXPORTS = ("lp_ray_samples_forward", "lp_ray_samples_backward", "lp_composite_forward", "lp_composite_backward")

#: every symbol include/lightplane_hip_importance.h declares (again a header and a table of their own)
IMPORTANCE_EXPORTS = ("lp_importance_samples_forward", "lp_importance_samples_backward")
#: the most coarse samples and the most new samples per ray (LP_IMPORTANCE_MAX of that header: a ray's working set stays in LDS)
LP_IMPORTANCE_MAX = 2048

#: every symbol include/lightplane_hip_losses.h declares (a header and a table of their own as well)
LOSSES_EXPORTS = ("lp_distortion_forward", "lp_distortion_backward", "lp_interlevel_forward", "lp_interlevel_backward")
#: the most samples (and proposal samples) per ray of the two losses (LP_RAY_LOSS_MAX of that header: a ray's working set stays in LDS)
LP_RAY_LOSS_MAX = 2048

#: every symbol include/lightplane_hip_render_samples.h declares (once more a header and a table of their own)
RENDER_SAMPLES_EXPORTS = ("lp_render_samples_forward", "lp_render_samples_backward", "lp_render_samples_chunks")

#: every symbol include/lightplane_hip_ray_grid.h declares (and once more)
RAY_GRID_EXPORTS = ("lp_ray_grid_splat", "lp_ray_grid_gather", "lp_ray_grid_grad_samples")


def _signatures():
    P, vp, i32, i64, f32 = C.POINTER, C.c_void_p, C.c_int32, C.c_int64, C.c_float
    ren, spl, tv_list = P(LpRendererArgs), P(LpSplatterArgs), P(LpGridList)
    tv = (tv_list, vp, i32, i32)          # grid-list, HOST weight array, count, p
    tv_grad = (vp, f32, vp, vp, i32)      # grad_loss, scale, grad, grad_list (HOST array), n_grad_list
    return (
        (("lp_version",), C.c_int, ()),
        (("lp_last_error", "lp_build_info"), C.c_char_p, ()),
        (("lp_abi_sizeof",), C.c_int, (C.c_int,)),
        (("lp_renderer_forward", "lp_renderer_backward"), C.c_int, (ren, vp)),
        (("lp_renderer_kernel_family", "lp_renderer_forward_family", "lp_renderer_backward_segments", "lp_renderer_relu_dump_words"),
         C.c_int, (ren,)),
        (("lp_renderer_forward_workspace_bytes",), i64, (ren,)),
        (("lp_renderer_forward_ws", "lp_renderer_backward_relu_dump"), C.c_int, (ren, vp, i64, vp)),
        (("lp_renderer_corner_rows",), C.c_int, (ren, vp, vp)),
        (("lp_splatter_forward", "lp_splatter_backward", "lp_mlp_splatter_launch_shape"), C.c_int, (spl, vp)),
        (("lp_splatter_kernel_family", "lp_mlp_splatter_relu_dump_words"), C.c_int, (spl,)),
        (("lp_mlp_splatter_backward_relu_dump",), C.c_int, (spl, vp, i64, vp)),
        (("lp_splatter_normalize",), C.c_int, (vp, vp, i64, i32, vp)),
        (("lp_hash_randn",), C.c_int, (vp, vp, vp, i64, i32, vp)),
        (("lp_ray_embedding_forward", "lp_ray_embedding_backward"), C.c_int, (P(LpRayEmbedArgs), vp)),
        # total-variation regulariser
        (("lp_grid_tv_workspace_bytes",), i64, (tv_list,)),
        (("lp_grid_tv_forward",), C.c_int, tv + (vp, vp, i64, vp)),
        (("lp_grid_tv_backward",), C.c_int, tv + tv_grad + (i32, vp)),
        (("lp_grid_tv_fused",), C.c_int, tv + (vp, vp, i64) + tv_grad + (vp,)),
        # resampling of a grid-list: source list, destination list, align_corners, HOST coefficient array (or NULL), ...
        (("lp_grid_resample_forward",), C.c_int, (tv_list, tv_list, i32, vp, vp)),
        (("lp_grid_resample_backward",), C.c_int, (tv_list, tv_list, i32, vp, i32, vp)),
        # occupancy scaffold of a grid-list: args, result (, workspace, workspace bytes), stream
        (("lp_scaffold_workspace_bytes",), i64, (P(LpScaffoldArgs),)),
        (("lp_scaffold_opacity",), C.c_int, (P(LpScaffoldArgs), vp, vp)),
        (("lp_scaffold_build",), C.c_int, (P(LpScaffoldArgs), vp, vp, i64, vp)),
        # the decoder at arbitrary points: args, stream
        (("lp_points_forward", "lp_points_backward"), C.c_int, (P(LpPointsArgs), vp)),
        # rays clipped to the occupied span of a scaffold: args, near_out, far_out, hit_out, stream
        (("lp_rays_clip",), C.c_int, (P(LpRayClipArgs), vp, vp, vp, vp)),
        # gather / splat of a grid-list at arbitrary points: args, stream
        (("lp_point_gather", "lp_point_splat", "lp_point_normalize", "lp_point_grad_points"), C.c_int, (P(LpPointGridArgs), vp)),
        # triangle mesh of a lattice's level set: args, workspace, workspace bytes, stream
        (("lp_mesh_workspace_bytes",), i64, (P(LpMeshArgs),)),
        (("lp_mesh_count", "lp_mesh_emit"), C.c_int, (P(LpMeshArgs), vp, i64, vp)),
        # sample placement and compositing of the march (include/lightplane_hip_samples.h): args, stream
        (SAMPLES_EXPORTS[:2], C.c_int, (P(LpRaySamplesArgs), vp)),
        (SAMPLES_EXPORTS[2:], C.c_int, (P(LpCompositeArgs), vp)),
        # importance resampling of a ray's samples (include/lightplane_hip_importance.h): args, stream
        (IMPORTANCE_EXPORTS, C.c_int, (P(LpImportanceArgs), vp)),
        # distortion and interlevel loss of a ray's samples (include/lightplane_hip_losses.h): args, stream
        (LOSSES_EXPORTS[:2], C.c_int, (P(LpDistortionArgs), vp)),
        (LOSSES_EXPORTS[2:], C.c_int, (P(LpInterlevelArgs), vp)),
        # decoder + compositing at caller-given depths (include/lightplane_hip_render_samples.h): args, stream; n_samples
        (RENDER_SAMPLES_EXPORTS[:2], C.c_int, (P(LpRenderSamplesArgs), vp)),
        (RENDER_SAMPLES_EXPORTS[2:], C.c_int, (i32,)),
        # weighted splat / gather of a grid-list along rays at caller-given depths (include/lightplane_hip_ray_grid.h): args, stream
        (RAY_GRID_EXPORTS, C.c_int, (P(LpRayGridArgs), vp)),
    )


#: ``(names, restype, argtypes)`` of every export: what ``lib()`` sets on the loaded library
SIGNATURES = _signatures()


class LightplaneHipError(RuntimeError):
    """A C-ABI call returned a non-zero code."""


def lib() -> C.CDLL:
    """Load (once) and return the HIP library; raise loudly if it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise LightplaneHipError(
            f"{LIB_PATH} not found: the HIP extension has not been built. Run "
            "`python lightplane_amd/csrc/build.py` (there is no CPU / PyTorch fallback)."
        )
    L = C.CDLL(LIB_PATH)
    for names, restype, argtypes in SIGNATURES:
        for name in names:
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, list(argtypes)
    for which, st in ((0, LpGrid), (1, LpGridList), (2, LpRays), (3, LpMarch), (4, LpMlp), (5, LpRendererArgs), (6, LpSplatterArgs),
                      (7, LpRayEmbedArgs), (8, LpScaffoldArgs), (10, LpPointsArgs), (12, LpRayClipArgs),
                      (14, LpPointGridArgs), (16, LpMeshArgs),  # (selectors 9, 11, 13 and 15 do not exist: lightplane_hip.h)
                      (18, LpRaySamplesArgs), (20, LpCompositeArgs),  # (nor 17, 19 and 21: lightplane_hip_samples.h)
                      (22, LpImportanceArgs),  # (nor 23: lightplane_hip_importance.h)
                      (24, LpDistortionArgs), (26, LpInterlevelArgs),  # (nor 25 and 27: lightplane_hip_losses.h)
                      (30, LpRenderSamplesArgs),  # (nor 28, 29 and 31: lightplane_hip_render_samples.h)
                      (34, LpRayGridArgs)):  # (nor 32, 33 and 35: lightplane_hip_ray_grid.h)
        if L.lp_abi_sizeof(which) != C.sizeof(st):
            raise LightplaneHipError(
                f"ABI mismatch: sizeof({st.__name__}) is {C.sizeof(st)} in the ctypes binding but "
                f"{L.lp_abi_sizeof(which)} in {LIB_PATH}; rebuild the library"
            )
    _LIB = L
    return L


def build_info() -> dict:
    """``lp_build_info()`` of the loaded library, parsed: version, ``src_hash`` (lightplane_amd/csrc/build.py ``source_hash()`` of the
    sources it was compiled from), compiler flags, and the arithmetic every backward family was compiled with."""
    import json
    return json.loads(lib().lp_build_info().decode())


def build_matches_tree() -> Optional[bool]:
    """True / False: the loaded library was built from the csrc/ + header of this tree (``src_hash``); None when the sources are
    not there to compare with (an installed binary)."""
    try:
        from .csrc import build as _b
        want = _b.source_hash()
    except Exception:
        return None
    return build_info().get("src_hash") == want


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().lp_last_error().decode(errors="replace")
        kind = {-1: "invalid argument", -2: "unsupported shape", -3: "NULL pointer"}.get(rc, f"hipError {rc}")
        err = LightplaneHipError(f"{what} failed ({kind}): {msg}")
        if rc in (-1, -3):
            # argument errors surface like the reference's Python-side asserts
            raise AssertionError(str(err))
        raise err


# --------------------------------------------------------------------------------------
# struct builders
# --------------------------------------------------------------------------------------


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    assert t.is_contiguous(), "tensors handed to the HIP library must be contiguous"
    return t.data_ptr()


_grid_clone_warned = False


def aligned(t: Optional[torch.Tensor], grid: bool = False) -> Optional[torch.Tensor]:
    """``t`` itself when its base is 16-byte aligned -- every fresh allocation is -- and otherwise a fresh contiguous clone.  Every
    device pointer of the C ABI has to be 16-byte aligned (include/lightplane_hip.h: the kernels move caller memory as float4 /
    float2, and the entry points refuse anything else); ``x.contiguous()`` does not move a view that is already dense, so
    ``buf[1:].view(shape)``, a parameter carved out of a flat parameter vector or ``rays.encoding[1:]`` would reach them at a 4-byte
    aligned base.  Applied after ``.contiguous()`` wherever a tensor's pointer goes to the library; inside the autograd functions, so
    that autograd still sees the caller's view.  ``grid=True``: the clone of a grid warns once per process -- for a multi-GB grid it is
    a cost the caller should hear about."""
    if t is None or t.data_ptr() % 16 == 0:
        return t
    if grid:
        global _grid_clone_warned
        if not _grid_clone_warned:
            _grid_clone_warned = True
            warnings.warn(
                f"lightplane_amd: a grid tensor of shape {tuple(t.shape)} starts at an address that is not 16-byte aligned (a view at an "
                "element offset into a larger buffer?) and is copied to an aligned buffer on every call (the copy stays allocated until the "
                "backward has run); allocate the grid on its own, or "
                "at a multiple of 4 floats into the buffer, to avoid the copy.  (Warned once per process.)", stacklevel=2)
    return t.clone(memory_format=torch.contiguous_format)


def check_tensors(device: torch.device, float32: dict, any_dtype: Optional[dict] = None) -> None:
    """Every tensor whose raw pointer goes to the HIP library has to live on ``device`` (the kernels dereference
    the pointers on that GPU: a CPU tensor or a tensor of another GPU would be a memory fault, not an exception)
    and -- for the ``float32`` group -- be fp32 (the kernels reinterpret the bytes).  ``None`` entries are skipped.
    Raises ``AssertionError`` like the reference's Python-side checks (lightplane_renderer.py:402-468)."""
    for group, need_f32 in ((float32, True), (any_dtype or {}, False)):
        for name, t in group.items():
            if t is None:
                continue
            assert torch.is_tensor(t), f"{name} has to be a tensor"
            assert t.device == device, (
                f"{name} is on {t.device} but the grid is on {device}: every tensor of a lightplane_amd call has to "
                f"live on the same GPU (forgot .to(device)?)")
            if need_f32:
                assert t.dtype == torch.float32, f"{name} has to be float32 (got {t.dtype})"


def check_grids(tensors, name: str, extra_f32: Optional[dict] = None, any_dtype: Optional[dict] = None,
                device: Optional[torch.device] = None) -> torch.device:
    """The checks of a front-end that hands grid tensors to the library as they are: ``extra_f32`` and the grids (``name[i]``) fp32,
    ``any_dtype`` of whatever type, all on ``device`` (default: the first grid's), the grids contiguous, and the device a GPU."""
    dev = tensors[0].device if device is None else device
    f32 = dict(extra_f32 or ())
    f32.update({f"{name}[{i}]": g for i, g in enumerate(tensors)})
    check_tensors(dev, f32, any_dtype)
    for g in tensors:
        assert g.is_contiguous(), "grids handed to the HIP library must be contiguous"
    current_stream(dev)  # (raises for anything but a GPU: there is no CPU path)
    return dev


def int32_index(t: torch.Tensor) -> torch.Tensor:
    """A ``grid_idx`` tensor as the kernels read it: int32, contiguous, 16-byte aligned."""
    return aligned(t.to(torch.int32).contiguous())


def query(fn, *args, what: str) -> int:
    """The count a ``*_workspace_bytes`` / ``*_dump_words`` style entry point answers; a negative answer is its error code."""
    n = int(fn(*args))
    if n < 0:
        check(n, what)
    return n


def current_stream(device: torch.device) -> Optional[int]:
    if device.type != "cuda":
        raise LightplaneHipError(
            f"lightplane_amd kernels run on the GPU only (got tensors on '{device}'); "
            "there is no CPU path -- the CPU oracle lives under oracle/ for tests."
        )
    raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)  # what Triton's launcher uses: no Stream object built
    if raw is not None:
        return raw(device.index if device.index is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(device).cuda_stream


def make_rays(directions, origins, grid_idx_i32, near, far, encoding, row_length: int = 0) -> LpRays:
    r = LpRays()
    r.row_length = int(row_length)
    r.n_rays = directions.shape[0]
    r.directions, r.origins = ptr(directions), ptr(origins)
    r.grid_idx, r.near_t, r.far_t = ptr(grid_idx_i32), ptr(near), ptr(far)
    r.encoding = ptr(encoding)
    r.encoding_dim = 0 if encoding is None else encoding.shape[1]
    return r


def make_march(num_samples, num_samples_inf, mask_out_of_bounds_samples, contract_coords, disparity_at_inf) -> LpMarch:
    m = LpMarch()
    m.num_samples, m.num_samples_inf = int(num_samples), int(num_samples_inf)
    m.mask_out_of_bounds = int(bool(mask_out_of_bounds_samples))
    m.contract_coords = int(bool(contract_coords))
    m.disparity_at_inf = float(disparity_at_inf)
    return m


def make_grid_list(data, descs: Sequence, channels: int, n_rows: int) -> LpGridList:
    """``data``: the flat ``[rows, C]`` tensor (grids at their ``row_offset``), or a LIST of per-grid tensors (zero-copy
    grid-lists: every grid in its own allocation, addressed from row 0 of its own tensor), or ``None`` (shapes only)."""
    gl = LpGridList()
    assert len(descs) <= LP_MAX_GRIDS, f"at most {LP_MAX_GRIDS} grids per grid-list are supported"
    per_grid = isinstance(data, (list, tuple))
    gl.data = None if per_grid else ptr(data)
    gl.n_grids = len(descs)
    gl.channels = int(channels)
    gl.n_rows = int(n_rows)
    for i, d in enumerate(descs):
        if per_grid:
            gl.grids[i] = LpGrid(d.B, d.D, d.H, d.W, 0, ptr(data[i]))
        else:
            gl.grids[i] = LpGrid(d.B, d.D, d.H, d.W, d.row_offset, None)
    return gl


def fill_ptr_list(field, tensors) -> None:
    """``field``: a ``c_void_p * LP_MAX_GRIDS`` array of an argument struct; entry g = pointer of ``tensors[g]``."""
    for i in range(LP_MAX_GRIDS):
        field[i] = ptr(tensors[i]) if (tensors is not None and i < len(tensors) and tensors[i] is not None) else None


def make_mlp(dims: Sequence[int], offset: int) -> LpMlp:
    m = LpMlp()
    dims = [int(v) for v in dims]
    n_layers = max(len(dims) - 1, 0)
    assert n_layers <= LP_MAX_LAYERS, f"at most {LP_MAX_LAYERS} layers per MLP are supported"
    m.n_layers = n_layers
    for i, v in enumerate(dims):
        m.dims[i] = v
    m.offset = int(offset)
    return m


def make_decoder(a, dims_t, dims_o, dims_c=None) -> None:
    """``a.trunk``, ``a.opacity`` and (with ``dims_c``) ``a.color``: the decoder's MLPs, one after the other in the flat parameter vector."""
    n_t = mlp_numel(dims_t)
    a.trunk, a.opacity = make_mlp(dims_t, 0), make_mlp(dims_o, n_t)
    if dims_c is not None:
        a.color = make_mlp(dims_c, n_t + mlp_numel(dims_o))


def route_grads(a, field: str, form, grads, needs, clear: bool = False) -> tuple:
    """Hand the gradient buffers of a grid-list (``grads``: one per tensor of ``form``, or ``None`` -- the kernels scatter into every
    grid of a list or into none, so the caller allocates all of them when any grid asks) to the argument block: a flat form's to
    ``a.<field>``, a list's to ``a.<field>_list``.  Returns what autograd gets: the buffers somebody asked for.  ``clear``: ``a`` is a
    used block, reset both fields."""
    flat = grads is not None and not form.is_list
    many = grads is not None and form.is_list
    if flat or clear:
        setattr(a, field, ptr(grads[0]) if flat else None)
    if many or clear:
        fill_ptr_list(getattr(a, field + "_list"), grads if many else None)
    if grads is None:
        return (None,) * len(needs)
    return tuple(g if need else None for g, need in zip(grads, needs))

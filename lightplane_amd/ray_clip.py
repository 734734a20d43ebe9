"""Rays clipped to the occupied span of a scaffold, fused into HIP (``csrc/lp_ray_clip.hip``; C ABI ``lp_rays_clip``).

The Renderer reads a scaffold ``[B, D, H, W]`` with nearest-neighbour, ``align_corners=False`` indexing, so scene ``b`` is tiled by
``W x H x D`` axis-aligned boxes -- cell ``i`` along x covers ``[-1 + 2 i / W, -1 + 2 (i + 1) / W]`` -- and a sample in a cell whose value
is 0 contributes nothing.  ``clip_rays_to_scaffold`` walks each ray through these cells (a 3-D DDA, one lane per ray) and returns the
ray batch with ``near`` / ``far`` shrunk to the span between the first and the last occupied cell the ray crosses inside its
``[near, far]`` and the scene box ``[-1, 1]^3``, widened by ``pad`` cells of the finest axis.  The result is conservative: no sample
the Renderer places on the original ``[near, far]`` outside the new span has a non-zero scaffold value.  Rendering
the clipped rays with proportionally fewer samples keeps the sample density; keeping the sample count raises it.  With
``num_samples_inf > 0`` the beyond-far samples start at the new ``far``.

No gradient (a span has none), no host synchronisation (graph-capturable), no atomics (bit-reproducible), no CPU path.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from . import _lib
from .rays import Rays

__all__ = ["clip_rays_to_scaffold"]


@torch.no_grad()
def clip_rays_to_scaffold(rays: Rays, scaffold: Optional[torch.Tensor] = None, *, pad: float = 0.5,
                          out: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None) -> Tuple[Rays, torch.Tensor]:
    """``(clipped rays, hit)``: ``rays`` with new ``near`` / ``far`` tensors (``directions``, ``origins``, ``grid_idx`` and ``encoding``
    are shared with the input) and a bool ``[R]`` tensor, False for a ray that crosses no occupied cell inside its ``[near, far]`` -- such
    a ray keeps its ``near`` / ``far`` bit for bit, as does one with ``far < near``, a NaN or Inf entry or a ``grid_idx`` outside the
    scaffold's batch.

    ``scaffold``: ``[B, D, H, W]`` fp32 (a cell is occupied iff its value ``!= 0``), or ``None`` to clip to the box ``[-1, 1]^3`` alone.
    ``pad``: margin in cells of the finest axis, ``pad * 2 / max(D, H, W) / |direction|`` in ray parameter (``2 / |direction|`` per unit
    without a scaffold).  ``out = (near, far, hit_uint8)``: preallocated contiguous results (fp32, fp32, uint8 ``[R]``), e.g. for graph
    capture; ``near`` / ``far`` may be the input's own tensors (in place)."""
    assert isinstance(rays, Rays), f"rays has to be a Rays object, got {type(rays).__name__}"
    pad = float(pad)
    assert pad >= 0.0 and pad != float("inf"), f"pad has to be >= 0 and finite, got {pad!r}"
    dev = rays.directions.device
    _lib.check_tensors(dev, {"rays.directions": rays.directions, "rays.origins": rays.origins, "rays.near": rays.near,
                             "rays.far": rays.far, "scaffold": scaffold}, {"rays.grid_idx": rays.grid_idx})
    if scaffold is not None:
        assert scaffold.ndim == 4 and scaffold.numel() > 0, f"scaffold has to be a non-empty [B, D, H, W] tensor, got {tuple(scaffold.shape)}"
        assert scaffold.is_contiguous(), "the scaffold handed to the HIP library must be contiguous"
    for name in ("directions", "origins", "near", "far", "grid_idx"):
        assert getattr(rays, name).is_contiguous(), f"rays.{name} handed to the HIP library must be contiguous"
    n = int(rays.directions.shape[0])
    stream = _lib.current_stream(dev)  # (raises for anything but a GPU: there is no CPU path)
    with torch.cuda.device(dev):
        if out is None:
            near, far = torch.empty_like(rays.near), torch.empty_like(rays.far)
            hit = torch.empty(n, dtype=torch.uint8, device=dev)
        else:
            near, far, hit = out
            _lib.check_tensors(dev, {"out[0]": near, "out[1]": far}, {"out[2]": hit})
            assert hit.dtype == torch.uint8, f"out[2] has to be uint8 (got {hit.dtype})"
            for i, t in enumerate((near, far, hit)):
                assert t.is_contiguous() and tuple(t.shape) == (n,), f"out[{i}] has to be a contiguous [{n}] tensor"
        a = _lib.LpRayClipArgs()
        directions, origins = _lib.aligned(rays.directions), _lib.aligned(rays.origins)
        grid_idx = _lib.int32_index(rays.grid_idx)
        near_in, far_in = rays.near, rays.far
        if near_in.data_ptr() % 16 and near_in is not near:
            near_in = _lib.aligned(near_in)
        if far_in.data_ptr() % 16 and far_in is not far:
            far_in = _lib.aligned(far_in)
        a.rays = _lib.make_rays(directions, origins, grid_idx, near_in, far_in, None)
        if scaffold is not None:
            scaffold = _lib.aligned(scaffold)
            a.scaffold = _lib.ptr(scaffold)
            a.scaffold_shape = _lib.LpGrid(*(int(v) for v in scaffold.shape), 0, None)
        a.pad = pad
        _lib.check(_lib.lib().lp_rays_clip(ctypes.byref(a), near.data_ptr(), far.data_ptr(), hit.data_ptr(), stream), "lp_rays_clip")
    clipped = Rays(directions=rays.directions, origins=rays.origins, grid_idx=rays.grid_idx, near=near, far=far, encoding=rays.encoding)
    return clipped, hit.bool()

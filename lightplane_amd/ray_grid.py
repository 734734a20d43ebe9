"""Weighted splat and gather of a grid-list along rays at caller-given sample depths, fused into HIP (``csrc/lp_ray_grid.hip``; C ABI
``lp_ray_grid_splat`` / ``lp_ray_grid_gather`` / ``lp_ray_grid_grad_samples`` of ``include/lightplane_hip_ray_grid.h``).

What a feed-forward 3D model lifts is a pixel feature times a depth distribution::

    grid += weights[r, s] * features[r]   at   origins[r] + depths[r, s] * directions[r]

and its dual renders a feature grid with given weights, ``out[r] = sum_s weights[r, s] * sample(grid, p_rs)``.  The depths are the
caller's: bins, ``importance_samples``, or the ``weights`` of ``render_samples(..., return_weights=True)``.  Through ``splat_points`` /
``sample_grid_at_points`` either costs an ``[R, S, C]`` tensor and its gradient; here no tensor of that size exists and the per-ray
vector is read once per ray.

For the grid-list ``G`` (``C`` channels), a per-ray vector ``F [R, C]``, ``p_rs = depths[r, s] * directions[r] + origins[r]``,
``q = contract(p)`` when asked, batch element ``rays.grid_idx[r]``::

    T(G, W, F; P) = sum_r sum_s W[r, s] sum over grids g and corners k of  w_k(q_rs) <G_g[row_k(q_rs)], F[r]>

with the corner rows and weights of ``point_grid`` (``align_corners=False``, zero padding; with ``mask_out_of_bounds_samples`` a point
outside ``[-1, 1]^3`` after the contraction adds nothing): the bilinear form ``B`` of ``point_grid`` with ``U[r, s] = W[r, s] F[r]``.
``splat_along_rays(normalize=False)`` is ``dT/dG``, ``gather_along_rays`` is ``dT/dF``, and every gradient of either is a partial
derivative of ``T`` again.  Grids go to the kernels as they are -- a list of tensors that is never concatenated or permuted, or the flat
``[sum BDHW, C]`` tensor with ``grid_sizes``.  Which gradients are computed follows ``requires_grad``; ``rays.origins`` and
``rays.directions`` get none.  Of ``rays`` only ``origins``, ``directions`` and ``grid_idx`` are read.  The gather and the sample
gradients are bit-reproducible; the splat accumulates with atomics.  fp32, no host synchronisation (graph-capturable), no double
backward, no CPU path.
"""
from __future__ import annotations

import ctypes
from typing import List, NamedTuple, Union

import torch

from . import _lib
from .grids import GridForm
from .rays import Rays

__all__ = ["splat_along_rays", "gather_along_rays"]


class _Cfg(NamedTuple):
    grid: GridForm
    mask: bool
    contract: bool
    normalize: bool = False


def _args(cfg: _Cfg, tensors, origins, directions, grid_idx, depths, weights, row_weight=None) -> _lib.LpRayGridArgs:
    """``tensors``: the grid-list's tensors in the form ``cfg`` describes; ``row_weight``: ``None`` or their ``[rows]`` twins."""
    a = _lib.LpRayGridArgs()
    form = cfg.grid
    a.grid = form.abi(tensors)
    if row_weight is not None:
        for g in range(len(form.descs)):  # (the flat form has one buffer: row i of the flat tensor has weight i)
            a.row_weight[g] = _lib.ptr(row_weight[g if form.is_list else 0])
    a.origins, a.directions, a.grid_idx = _lib.ptr(origins), _lib.ptr(directions), _lib.ptr(grid_idx)
    a.depths, a.weights = _lib.ptr(depths), _lib.ptr(weights)
    a.n_rays, a.n_samples = depths.shape
    a.channels = form.channels
    a.mask_out_of_bounds, a.contract_coords = int(cfg.mask), int(cfg.contract)
    return a


def _call(name: str, a, stream) -> None:
    _lib.check(getattr(_lib.lib(), name)(ctypes.byref(a), stream), name)


def _dense(t: torch.Tensor) -> torch.Tensor:
    return _lib.aligned(t.to(torch.float32).contiguous())


def _grad_samples(cfg, tensors, ray, depths, weights, vectors, want_w: bool, want_d: bool, stream):
    """``(dT/dW, dT/d depths)`` of the grid-list ``tensors`` and the per-ray ``vectors``: one launch, the one nobody wants is skipped."""
    empty = depths.numel() == 0  # (nothing is launched: the results are empty, or there is no ray)
    d_w = (torch.zeros_like(depths) if empty else torch.empty_like(depths)) if want_w else None
    d_d = (torch.zeros_like(depths) if empty else torch.empty_like(depths)) if want_d else None
    if (want_w or want_d) and not empty:
        a = _args(cfg, tensors, *ray, depths, weights)
        a.vectors, a.grad_weights, a.grad_depths = _lib.ptr(vectors), _lib.ptr(d_w), _lib.ptr(d_d)
        _call("lp_ray_grid_grad_samples", a, stream)
    return d_w, d_d


def _gather(cfg, tensors, ray, depths, weights, row_weight, stream):
    n, s = depths.shape
    out = (torch.zeros if n * s == 0 else torch.empty)(n, cfg.grid.channels, device=depths.device, dtype=torch.float32)
    if n * s > 0:
        a = _args(cfg, tensors, *ray, depths, weights, row_weight)
        a.out_features = _lib.ptr(out)
        _call("lp_ray_grid_gather", a, stream)
    return out


class _GatherAlongRays(torch.autograd.Function):
    """out = dT/dF: one launch, no atomics.  Backward: the splat of the upstream gradient as the per-ray vector into zeroed twins of the
    grids (when a grid asks) and the stored sample gradients (when ``weights`` or ``depths`` ask) -- a kernel nobody asks for does not
    run."""

    @staticmethod
    def forward(ctx, cfg: _Cfg, origins, directions, grid_idx, depths, weights, *tensors):
        dev = depths.device
        stream = _lib.current_stream(dev)
        origins, directions, depths, weights = (_lib.aligned(t.contiguous()) for t in (origins, directions, depths, weights))
        tensors = tuple(_lib.aligned(t, grid=True) for t in tensors)
        with torch.cuda.device(dev):
            out = _gather(cfg, tensors, (origins, directions, grid_idx), depths, weights, None, stream)
        ctx.cfg = cfg
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(origins, directions, grid_idx, depths, weights, *tensors)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        cfg: _Cfg = ctx.cfg
        origins, directions, grid_idx, depths, weights, *tensors = ctx.saved_tensors
        need = ctx.needs_input_grad
        n_in = 6 + len(tensors)
        if g_out is None or not any(need):
            return (None,) * n_in
        dev = depths.device
        stream = _lib.current_stream(dev)
        g_out = _dense(g_out)
        ray = (origins, directions, grid_idx)
        d_grids = None
        with torch.cuda.device(dev):
            d_w, d_d = _grad_samples(cfg, tensors, ray, depths, weights, g_out, need[5], need[4], stream)
            if any(need[6:]):  # (the kernel scatters into every grid of the list)
                d_grids = [torch.zeros_like(t) for t in tensors]
                if depths.numel() > 0:
                    a = _args(cfg, d_grids, *ray, depths, weights)
                    a.vectors = _lib.ptr(g_out)
                    _call("lp_ray_grid_splat", a, stream)
        grads = [g if n else None for g, n in zip(d_grids or [None] * len(tensors), need[6:])]
        return (None, None, None, None, d_d, d_w, *grads)


class _SplatAlongRays(torch.autograd.Function):
    """grid-list = dT/dG into zeroed tensors (one launch; with ``normalize`` the coefficients go to ``[rows]`` buffers in the same launch
    and ``lp_point_normalize`` divides in place).  Backward: the gather of the upstream grids -- divided by the saved weights as they
    are read when normalised -- and, for the raw splat, the stored sample gradients."""

    @staticmethod
    def forward(ctx, cfg: _Cfg, origins, directions, grid_idx, depths, weights, features):
        dev = depths.device
        stream = _lib.current_stream(dev)
        origins, directions, depths, weights, features = (
            _lib.aligned(t.contiguous()) for t in (origins, directions, depths, weights, features))
        with torch.cuda.device(dev):
            outs = [torch.zeros(s, device=dev, dtype=torch.float32) for s in cfg.grid.out_shapes()]
            row_w = [torch.zeros(o.numel() // o.shape[-1], device=dev, dtype=torch.float32) for o in outs] if cfg.normalize else None
            if depths.numel() > 0:
                a = _args(cfg, outs, origins, directions, grid_idx, depths, weights, row_w)
                a.vectors = _lib.ptr(features)
                _call("lp_ray_grid_splat", a, stream)
                if cfg.normalize:  # (the division of the point ops, as it is: it looks at the grids and their weights only)
                    pa = _lib.LpPointGridArgs()
                    pa.grid, pa.row_weight, pa.channels = a.grid, a.row_weight, a.channels
                    pa.n_rays = pa.n_pts = 1  # (not an empty batch: something was splatted)
                    _call("lp_point_normalize", pa, stream)
        ctx.cfg = cfg
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(origins, directions, grid_idx, depths, weights, features, *(row_w or ()))
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *g_outs):
        cfg: _Cfg = ctx.cfg
        origins, directions, grid_idx, depths, weights, features, *row_w = ctx.saved_tensors
        need = ctx.needs_input_grad
        if all(g is None for g in g_outs) or not any(need):
            return (None,) * 7
        dev = depths.device
        stream = _lib.current_stream(dev)
        ray = (origins, directions, grid_idx)
        with torch.cuda.device(dev):
            # (a grid nobody differentiated has a zero upstream gradient: the kernels read every grid of the list)
            ups = [torch.zeros(s, device=dev, dtype=torch.float32) if g is None else _dense(g)
                   for g, s in zip(g_outs, cfg.grid.out_shapes())]
            d_features = _gather(cfg, ups, ray, depths, weights, row_w if cfg.normalize else None, stream) if need[6] else None
            assert not (cfg.normalize and (need[4] or need[5]))  # (splat_along_rays refuses it)
            d_w, d_d = _grad_samples(cfg, ups, ray, depths, weights, features, need[5], need[4], stream)
        return None, None, None, None, d_d, d_w, d_features


def _check_rays(rays, depths, weights):
    assert isinstance(rays, Rays), f"rays has to be a Rays object, got {type(rays).__name__}"
    assert torch.is_tensor(depths) and depths.ndim == 2, "depths has to be a [n_rays, n_samples] tensor"
    n, s = depths.shape
    assert torch.is_tensor(weights) and tuple(weights.shape) == (n, s), f"weights has to be a [{n}, {s}] tensor, as depths is"
    assert n * s < 2 ** 31, f"depths: {n} rays x {s} samples: n_rays * n_samples has to stay below 2^31 (split the batch)"
    for name, t in (("rays.origins", rays.origins), ("rays.directions", rays.directions)):
        assert torch.is_tensor(t) and tuple(t.shape) == (n, 3), f"{name} has to be a [{n}, 3] tensor: one ray per row of depths"
    idx = rays.grid_idx
    assert torch.is_tensor(idx) and tuple(idx.shape) == (n,), f"rays.grid_idx has to be a [{n}] tensor"
    if torch.is_grad_enabled():
        for name, t in (("rays.origins", rays.origins), ("rays.directions", rays.directions)):
            if t.requires_grad:
                raise NotImplementedError(
                    f"{name} requires a gradient, and the ops along rays produce none for ray origins and directions: pass "
                    f"{name}.detach(), or form the points yourself, o + t·d → splat_points / sample_grid_at_points, which differentiates "
                    "them")


def splat_along_rays(rays: Rays, depths: torch.Tensor, weights: torch.Tensor, features: torch.Tensor, output_grid_size, *,
                     mask_out_of_bounds_samples: bool = False, contract_coords: bool = False, normalize: bool = False,
                     return_list: bool = True) -> Union[List[torch.Tensor], torch.Tensor]:
    """Lift the per-ray ``features [R, C]`` along ``rays`` into a grid-list of the sizes ``output_grid_size`` (a list of
    ``[B, D, H, W, C]``): ``weights[r, s] * w_k * features[r]`` is added to the corner rows of every grid at
    ``rays.origins[r] + depths[r, s] * rays.directions[r]`` (``depths``, ``weights`` ``[R, S]`` fp32, any values in any order).

    ``normalize=False``: the raw sums ``dT/dG`` (module docstring), differentiable with respect to ``features``, ``weights`` and
    ``depths``.  ``normalize=True``: every row divided by its splatted weight ``sum weights * w_k``, clamped at ``1e-5`` -- with
    ``weights = 1`` at the depths of ``ray_samples`` the ``lightplane_splatter`` result; differentiable with respect to ``features``
    only (the derivative through the division is not provided: ``weights`` and ``depths`` must not require a gradient).  Returns the
    list of ``[B, D, H, W, C]`` tensors, or with ``return_list=False`` the flat ``[sum BDHW, C]`` tensor (splatted into directly)."""
    _check_rays(rays, depths, weights)
    form = GridForm.of_sizes(output_grid_size, sampler=False, is_list=bool(return_list))
    n = depths.shape[0]
    assert torch.is_tensor(features) and tuple(features.shape) == (n, form.channels), (
        f"features has to be a [{n}, {form.channels}] tensor (one vector per ray, the grids' channels)")
    if normalize and torch.is_grad_enabled():
        for name, t in (("weights", weights), ("depths", depths)):
            if t.requires_grad:
                raise NotImplementedError(
                    f"splat_along_rays(normalize=True) has no gradient with respect to {name} (the derivative through the division by "
                    f"the splatted weights is not provided): use normalize=False, or detach the {name}")
    f32 = {"depths": depths, "weights": weights, "features": features, "rays.origins": rays.origins, "rays.directions": rays.directions}
    _lib.check_grids((), "grid", f32, {"rays.grid_idx": rays.grid_idx}, device=depths.device)
    grid_idx = _lib.int32_index(rays.grid_idx)
    cfg = _Cfg(form, bool(mask_out_of_bounds_samples), bool(contract_coords), bool(normalize))
    outs = _SplatAlongRays.apply(cfg, rays.origins.detach(), rays.directions.detach(), grid_idx, depths, weights, features)
    return list(outs) if return_list else outs[0]


def gather_along_rays(rays: Rays, depths: torch.Tensor, weights: torch.Tensor, grid, *, mask_out_of_bounds_samples: bool = False,
                      contract_coords: bool = False, grid_sizes=None) -> torch.Tensor:
    """``out [R, C] = sum_s weights[r, s] * sample(grid, rays.origins[r] + depths[r, s] * rays.directions[r])``: the grid-list rendered
    along ``rays`` with the caller's weights (``dT/dF`` of the module docstring; ``depths``, ``weights`` ``[R, S]`` fp32).

    ``grid``: a *list* of ``[B, D, H, W, C]`` tensors, or a flat ``[sum BDHW, C]`` tensor with ``grid_sizes``, as
    ``sample_grid_at_points`` takes them.  Differentiable with respect to every grid, ``weights`` and ``depths``.  Bit-reproducible."""
    _check_rays(rays, depths, weights)
    tensors, form = GridForm.of(grid, grid_sizes, name="grid", sampler=False)
    f32 = {"depths": depths, "weights": weights, "rays.origins": rays.origins, "rays.directions": rays.directions}
    _lib.check_grids(tensors, "grid", f32, {"rays.grid_idx": rays.grid_idx}, device=depths.device)
    grid_idx = _lib.int32_index(rays.grid_idx)
    cfg = _Cfg(form, bool(mask_out_of_bounds_samples), bool(contract_coords))
    return _GatherAlongRays.apply(cfg, rays.origins.detach(), rays.directions.detach(), grid_idx, depths, weights, *tensors)

"""Gather and splat of a grid-list at arbitrary 3-D points, fused into HIP (``csrc/lp_point_grid.hip``; C ABI ``lp_point_gather`` /
``lp_point_splat`` / ``lp_point_normalize`` / ``lp_point_grad_points``).  The counterpart at points of the Renderer's gather and the
Splatter's scatter along rays, without a decoder behind it.

For the grid-list ``G``, points ``P [R, N, 3]``, per-point vectors ``U [R, N, C]``, ``q = contract(p)`` when asked, batch element
``ray_grid_idx[r]`` for every point of row ``r``::

    B(G, P, U) = sum over points, grids g and corners k of  w_k(q) <G_g[row_k(q)], U[point]>

with the Renderer's corner rows and tri- / bi-linear weights (``align_corners=False``, zero padding; with
``mask_out_of_bounds_samples`` a point outside ``[-1, 1]^3`` contributes nothing).  ``sample_grid_at_points`` is ``dB/dU``,
``splat_points(normalize=False)`` is ``dB/dG``, and every gradient of either is one of the three partial derivatives again: the gather's
gradient into the grids is the splat of the upstream gradient, the splat's gradient into the features is the gather of the upstream
grids, and both point gradients are ``dB/dP`` (the derivative of the interpolation weights, through the Jacobian of the contraction;
the mask is piecewise constant).  Grids go to the kernels as they are -- a list of tensors that is never concatenated or permuted, or
the flat ``[sum BDHW, C]`` tensor with ``grid_sizes``.  Which gradients are computed follows ``requires_grad``; there is no double
backward and no CPU path.  No host synchronisation (graph-capturable).
"""
from __future__ import annotations

import ctypes
from typing import List, NamedTuple, Union

import torch

from . import _lib
from .grids import GridForm

__all__ = ["sample_grid_at_points", "splat_points"]


class _Cfg(NamedTuple):
    grid: GridForm
    mask: bool
    contract: bool
    normalize: bool = False


def _args(cfg: _Cfg, tensors, points, grid_idx, row_weight=None) -> _lib.LpPointGridArgs:
    """``tensors``: the grid-list's tensors in the form ``cfg`` describes; ``row_weight``: ``None`` or their ``[rows]`` twins."""
    a = _lib.LpPointGridArgs()
    form = cfg.grid
    a.grid = form.abi(tensors)
    if row_weight is not None:
        for g in range(len(form.descs)):  # (the flat form has one buffer: row i of the flat tensor has weight i)
            a.row_weight[g] = _lib.ptr(row_weight[g if form.is_list else 0])
    a.points, a.grid_idx = _lib.ptr(points), _lib.ptr(grid_idx)
    a.n_rays, a.n_pts = points.shape[0], points.shape[1]
    a.channels = form.channels
    a.mask_out_of_bounds, a.contract_coords = int(cfg.mask), int(cfg.contract)
    return a


def _call(name: str, a: _lib.LpPointGridArgs, stream) -> None:
    _lib.check(getattr(_lib.lib(), name)(ctypes.byref(a), stream), name)


def _dense(t: torch.Tensor) -> torch.Tensor:
    return _lib.aligned(t.to(torch.float32).contiguous())


class _SampleAtPoints(torch.autograd.Function):
    """features = gather(grids, points): one launch, no atomics.  Backward: the splat of the upstream gradient into zeroed twins of the
    grids (when a grid asks) and the stored point gradient (when ``points`` asks) -- a kernel nobody asks for does not run."""

    @staticmethod
    def forward(ctx, cfg: _Cfg, points, grid_idx, *tensors):
        dev = points.device
        stream = _lib.current_stream(dev)
        points = _lib.aligned(points.contiguous())
        tensors = tuple(_lib.aligned(t, grid=True) for t in tensors)
        with torch.cuda.device(dev):
            out = torch.empty(points.shape[0], points.shape[1], cfg.grid.channels, device=dev, dtype=torch.float32)
            a = _args(cfg, tensors, points, grid_idx)
            a.out_features = _lib.ptr(out)
            _call("lp_point_gather", a, stream)
        ctx.cfg = cfg
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(points, grid_idx, *tensors)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        cfg: _Cfg = ctx.cfg
        points, grid_idx, *tensors = ctx.saved_tensors
        need = ctx.needs_input_grad
        if g_out is None or not any(need):
            return (None,) * (3 + len(tensors))
        dev = points.device
        stream = _lib.current_stream(dev)
        g_out = _dense(g_out)
        d_points, d_grids = None, None
        with torch.cuda.device(dev):
            if need[1]:
                d_points = torch.empty_like(points)
                a = _args(cfg, tensors, points, grid_idx)
                a.vectors, a.grad_points = _lib.ptr(g_out), _lib.ptr(d_points)
                _call("lp_point_grad_points", a, stream)
            if any(need[3:]):  # (the kernel scatters into every grid of the list)
                d_grids = [torch.zeros_like(t) for t in tensors]
                a = _args(cfg, d_grids, points, grid_idx)
                a.vectors = _lib.ptr(g_out)
                _call("lp_point_splat", a, stream)
        grads = [g if n else None for g, n in zip(d_grids or [None] * len(tensors), need[3:])]
        return (None, d_points, None, *grads)


class _SplatPoints(torch.autograd.Function):
    """grid-list = splat(points, features) into zeroed tensors (one launch; with ``normalize`` the weights go to ``[rows]`` buffers in the
    same launch and a second one divides in place).  Backward: the gather of the upstream grids -- divided by the saved weights as they
    are read when normalised -- and, for the raw splat, the stored point gradient."""

    @staticmethod
    def forward(ctx, cfg: _Cfg, points, features, grid_idx):
        dev = points.device
        stream = _lib.current_stream(dev)
        points, features = _lib.aligned(points.contiguous()), _lib.aligned(features.contiguous())
        with torch.cuda.device(dev):
            outs = [torch.zeros(s, device=dev, dtype=torch.float32) for s in cfg.grid.out_shapes()]
            weights = [torch.zeros(o.numel() // o.shape[-1], device=dev, dtype=torch.float32) for o in outs] if cfg.normalize else None
            a = _args(cfg, outs, points, grid_idx, weights)
            a.vectors = _lib.ptr(features)
            _call("lp_point_splat", a, stream)
            if cfg.normalize:
                _call("lp_point_normalize", a, stream)
        ctx.cfg = cfg
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(points, features, grid_idx, *(weights or ()))
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *g_outs):
        cfg: _Cfg = ctx.cfg
        points, features, grid_idx, *weights = ctx.saved_tensors
        need = ctx.needs_input_grad
        if all(g is None for g in g_outs) or not (need[1] or need[2]):
            return None, None, None, None
        dev = points.device
        stream = _lib.current_stream(dev)
        d_points, d_features = None, None
        with torch.cuda.device(dev):
            # (a grid nobody differentiated has a zero upstream gradient: the kernels read every grid of the list)
            ups = [torch.zeros(s, device=dev, dtype=torch.float32) if g is None else _dense(g) for g, s in zip(g_outs, cfg.grid.out_shapes())]
            if need[2]:
                d_features = torch.empty_like(features)
                a = _args(cfg, ups, points, grid_idx, weights if cfg.normalize else None)
                a.out_features = _lib.ptr(d_features)
                _call("lp_point_gather", a, stream)
            if need[1]:
                assert not cfg.normalize  # (splat_points refuses it)
                d_points = torch.empty_like(points)
                a = _args(cfg, ups, points, grid_idx)
                a.vectors, a.grad_points = _lib.ptr(features), _lib.ptr(d_points)
                _call("lp_point_grad_points", a, stream)
        return None, d_points, d_features, None


def _check_points(points, ray_grid_idx):
    assert torch.is_tensor(points) and points.ndim == 3 and points.shape[-1] == 3, "points has to be a [n_rays, n_pts, 3] tensor"
    n_rays = points.shape[0]
    assert torch.is_tensor(ray_grid_idx) and tuple(ray_grid_idx.shape) == (n_rays,), f"ray_grid_idx has to be a [{n_rays}] tensor"
    assert not ray_grid_idx.is_floating_point() and not ray_grid_idx.is_complex() and ray_grid_idx.dtype != torch.bool, (
        "ray_grid_idx has to have an integer dtype")


def sample_grid_at_points(points, grid, ray_grid_idx, mask_out_of_bounds_samples: bool = False, contract_coords: bool = False, *,
                          grid_sizes=None) -> torch.Tensor:
    """``features [n_rays, n_pts, C]``: the sum over the grid-list of its tri- / bi-linear samples at ``points [n_rays, n_pts, 3]``
    (module docstring for the definition) -- what the Renderer and ``lightplane_eval_mlp`` feed their decoder.

    ``grid``: a *list* of ``[B, D, H, W, C]`` tensors, or a flat ``[sum BDHW, C]`` tensor with ``grid_sizes``, as
    ``lightplane_eval_mlp`` takes them; ``ray_grid_idx [n_rays]`` (any integer dtype): the batch element of each row's points.
    Differentiable with respect to every grid and to ``points``."""
    _check_points(points, ray_grid_idx)
    tensors, form = GridForm.of(grid, grid_sizes, name="grid", sampler=False)
    _lib.check_grids(tensors, "grid", {"points": points}, {"ray_grid_idx": ray_grid_idx}, device=points.device)
    grid_idx = _lib.int32_index(ray_grid_idx)
    cfg = _Cfg(form, bool(mask_out_of_bounds_samples), bool(contract_coords))
    return _SampleAtPoints.apply(cfg, points, grid_idx, *tensors)


def splat_points(points, features, output_grid_size, ray_grid_idx, mask_out_of_bounds_samples: bool = False,
                 contract_coords: bool = False, *, normalize: bool = True,
                 return_list: bool = True) -> Union[List[torch.Tensor], torch.Tensor]:
    """Lift the point cloud ``points [n_rays, n_pts, 3]`` with ``features [n_rays, n_pts, C]`` into a grid-list of the sizes
    ``output_grid_size`` (a list of ``[B, D, H, W, C]``): ``features[point] * w_k`` is added to the corner rows of every grid.

    ``normalize=True``: the ``lightplane_splatter`` result -- every row divided by its splatted weight, clamped at ``1e-5``;
    differentiable with respect to ``features`` (a point gradient through the division is not provided: ``points`` must not require
    one).  ``normalize=False``: the raw sums, the exact adjoint of ``sample_grid_at_points``; differentiable with respect to ``features``
    and ``points``.  Returns the list of ``[B, D, H, W, C]`` tensors, or with ``return_list=False`` the flat ``[sum BDHW, C]`` tensor
    (splatted into directly).  A per-ray ``[n_rays, C]`` feature is not broadcast: use the Splatter, or ``expand(...).contiguous()``."""
    _check_points(points, ray_grid_idx)
    form = GridForm.of_sizes(output_grid_size, sampler=False, is_list=bool(return_list))
    channels = form.channels
    assert torch.is_tensor(features) and tuple(features.shape) == tuple(points.shape[:2]) + (channels,), (
        f"features has to be a [{points.shape[0]}, {points.shape[1]}, {channels}] tensor (one vector per point, the grids' channels)")
    if normalize and points.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("splat_points(normalize=True) has no gradient with respect to points (the derivative through the "
                                  "division by the splatted weights is not provided): use normalize=False, or detach the points")
    _lib.check_grids((), "grid", {"points": points, "features": features}, {"ray_grid_idx": ray_grid_idx}, device=points.device)
    grid_idx = _lib.int32_index(ray_grid_idx)
    cfg = _Cfg(form, bool(mask_out_of_bounds_samples), bool(contract_coords), bool(normalize))
    outs = _SplatPoints.apply(cfg, points, features, grid_idx)
    return list(outs) if return_list else outs[0]

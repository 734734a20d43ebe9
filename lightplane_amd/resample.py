"""Resampling of a grid-list to new spatial sizes, fused into HIP sweeps (``csrc/lp_grid_resample.hip``; C ABI ``lp_grid_resample_*``).

Every grid ``[B, D, H, W, C]`` of the list is interpolated tri-linearly (a plane bi-linearly: a singular axis replicates) to new
``[D', H', W']``; batch and channels are never resampled.  Per axis, with one fp32 coefficient ``a``::

    align_corners:      src(o) = a * o                          a = (n_in - 1) / (n_out - 1)   (0 if n_out == 1)
    otherwise:          src(o) = max(0, a * (o + 0.5) - 0.5)    a = float(1 / scale_factor), or n_in / n_out when sizes are given
    i0 = min(floor(src), n_in - 1),  i1 = min(i0 + 1, n_in - 1),  lam = clamp(src - i0, 0, 1)

i.e. ``F.interpolate(g.permute(0, 4, 1, 2, 3), ...).permute(0, 2, 3, 4, 1).contiguous()`` -- the reference's ``grid_up_sample``
(examples/utils/util/grid_util.py) -- without the two layout copies, on the layouts the kernels take (a list of tensors that is never
concatenated, or the flat ``[sum BDHW, C]`` tensor with ``grid_sizes``), and differentiable: the backward is the adjoint sweep, a gather
without atomics (bit-reproducible).  No host synchronisation (graph-capturable); allocates the result and nothing else.
"""
from __future__ import annotations

import ctypes
import math
from typing import List, Optional

import torch

from . import _lib
from .grids import GridForm

__all__ = ["grid_resample", "grid_up_sample", "resampled_sizes"]


def resampled_sizes(grid_sizes, scale_factor: float) -> List[List[int]]:
    """``[B, D', H', W', C]`` of every grid after resampling by ``scale_factor``: ``floor(n * factor)`` on the axes with ``n > 1``; a
    singular axis stays singular (a plane stays a plane)."""
    f = float(scale_factor)
    assert f > 0.0 and math.isfinite(f), f"scale_factor has to be positive and finite, got {scale_factor!r}"
    out = []
    for gs in grid_sizes:
        gs = [int(v) for v in gs]
        assert len(gs) == 5, f"each grid size has to be [B, D, H, W, C], got {gs}"
        new = [gs[0]] + [n if n == 1 else int(math.floor(n * f)) for n in gs[1:4]] + [gs[4]]
        assert all(v >= 1 for v in new), f"scale_factor {f} leaves grid {gs} with an empty axis: {new}"
        out.append(new)
    return out


def _target_sizes(in_sizes, sizes, scale_factor) -> List[List[int]]:
    assert (sizes is None) != (scale_factor is None), "exactly one of sizes and scale_factor has to be given"
    if scale_factor is not None:
        return resampled_sizes(in_sizes, scale_factor)
    if torch.is_tensor(sizes):
        sizes = sizes.tolist()
    sizes = list(sizes)
    if len(sizes) == 3 and not isinstance(sizes[0], (list, tuple)):
        sizes = [sizes] * len(in_sizes)  # one [D, H, W] for every grid
    assert len(sizes) == len(in_sizes), f"sizes has {len(sizes)} entries for {len(in_sizes)} grids"
    out = []
    for gs, s in zip(in_sizes, sizes):
        s = [int(v) for v in s]
        assert len(s) == 3 and all(v >= 1 for v in s), f"each target size has to be a positive [D, H, W], got {s}"
        out.append([gs[0]] + s + [gs[4]])
    return out


def _coeffs(n_grids: int, scale_factor, align_corners: bool):
    """HOST coefficient array for the C ABI, or ``None`` (= derived from the sizes by the library).  Only a scale factor without
    ``align_corners`` sets the coordinate mapping itself -- ``float(1 / scale_factor)``, as ``F.interpolate`` has it, which differs
    from ``n_in / n_out`` whenever ``n * factor`` is not an integer."""
    if scale_factor is None or align_corners:
        return None
    a = 1.0 / float(scale_factor)
    return (ctypes.c_float * (3 * n_grids))(*([a] * (3 * n_grids)))




class _GridResample(torch.autograd.Function):
    """outputs = R(grid tensors): forward = one output-stationary sweep per grid into freshly allocated results; backward = one gather
    sweep per grid that WRITES one gradient per input tensor (no zero-fill, no atomics)."""

    @staticmethod
    def forward(ctx, cfg, *tensors):
        form, out_form, align, scale = cfg
        dev = tensors[0].device
        src = form.abi(tensors)
        with torch.cuda.device(dev):
            outs = tuple(torch.empty(s, dtype=torch.float32, device=dev) for s in out_form.out_shapes())
            dst = out_form.abi(outs)
            _lib.check(_lib.lib().lp_grid_resample_forward(ctypes.byref(src), ctypes.byref(dst), int(align),
                                                           _coeffs(len(form.descs), scale, align), _lib.current_stream(dev)),
                       "lp_grid_resample_forward")
        ctx.cfg = cfg
        return outs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *g_outs):
        form, out_form, align, scale = ctx.cfg
        if not any(ctx.needs_input_grad[1:]):
            return (None,) * (1 + form.n_tensors)
        dev = g_outs[0].device
        g_outs = tuple(g.to(dtype=torch.float32).contiguous() for g in g_outs)
        with torch.cuda.device(dev):
            grads = tuple(torch.empty(s, dtype=torch.float32, device=dev) for s in form.out_shapes())
            g_src, g_dst = form.abi(grads), out_form.abi(g_outs)
            _lib.check(_lib.lib().lp_grid_resample_backward(ctypes.byref(g_src), ctypes.byref(g_dst), int(align),
                                                            _coeffs(len(form.descs), scale, align), 0, _lib.current_stream(dev)),
                       "lp_grid_resample_backward")
        return (None,) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[1:]))


def grid_resample(grid, grid_sizes=None, *, sizes=None, scale_factor: Optional[float] = None, align_corners: bool = False):
    """Resample every grid of a grid-list to new spatial sizes (module docstring for the definition); differentiable.

    ``grid``: a *list* of ``[B, D, H, W, C]`` tensors or a flat ``[sum BDHW, C]`` tensor with ``grid_sizes``, as ``lightplane_renderer``
    takes them (anything else: ``NotImplementedError``).  Exactly one of ``sizes`` -- ``[D', H', W']`` per grid, or one triple for all --
    and ``scale_factor`` (outputs ``floor(n * factor)``, singular axes stay singular: ``resampled_sizes``).
    Returns the same container kind: a list of tensors, or ``(flat, new_grid_sizes)`` with the sizes as a list of ``[B, D', H', W', C]``.
    The backward returns one gradient per input tensor."""
    tensors, form = GridForm.of(grid, grid_sizes, sampler=False)
    out_sizes = _target_sizes(form.sizes(), sizes, scale_factor)
    out_form = GridForm.of_sizes(out_sizes, sampler=False, is_list=form.is_list)
    _lib.check_grids(tensors, "grid")
    cfg = (form, out_form, bool(align_corners), None if scale_factor is None else float(scale_factor))
    outs = _GridResample.apply(cfg, *tensors)
    if form.is_list:
        return list(outs)
    return outs[0], out_sizes


def grid_up_sample(grids: List[torch.Tensor], upsample_factor: float = 2.0, align_corners: bool = False) -> List[torch.Tensor]:
    """The reference's ``grid_up_sample`` (examples/utils/util/grid_util.py): replaces every entry of the list ``grids``, in place, by
    its resampling by ``upsample_factor`` -- a contiguous leaf with ``requires_grad=True``; a plane stays a plane -- and returns the
    list.  Runs without autograd: rebuild the optimiser for the new tensors afterwards."""
    assert isinstance(grids, list), "grid_up_sample takes a list of [B, D, H, W, C] tensors and replaces its entries"
    with torch.no_grad():
        new = grid_resample(list(grids), scale_factor=upsample_factor, align_corners=align_corners)
    for i, g in enumerate(new):
        grids[i] = g.requires_grad_(True)
    return grids

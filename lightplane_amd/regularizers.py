"""Regularisers of a grid-list, fused into HIP sweeps (``csrc/lp_grid_tv.hip``; C ABI ``lp_grid_tv_*``).

Total variation of one grid ``x`` of shape ``[B, D, H, W, C]``, ``p`` in {1, 2} (``phi_1(d) = |d|``, ``phi_2(d) = d ** 2``)::

    T_a    = sum of phi_p(x[.., i + 1, ..] - x[.., i, ..]) over the adjacent pairs along spatial axis a, all B, all C
    loss_g = sum over the axes a of (D, H, W) with extent > 1 of T_a / (number of those pairs)
    loss   = sum_g grid_weights[g] * loss_g

i.e. ``(g[:, 1:] - g[:, :-1]).abs().mean()`` per axis, summed -- without the full-size temporaries that expression makes and keeps
for autograd, and on the layouts the kernels take: a list of ``[B, D, H, W, C]`` tensors that is never concatenated, or the flat
``[sum BDHW, C]`` tensor with ``grid_sizes``.  A plane ``[B, 1, H, W, C]`` gets the 2-D TV of its plane; the derivative of ``|d|``
at 0 is 0, as ``torch.abs`` has it.  No atomics (bit-reproducible), no host synchronisation (graph-capturable).
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch

from . import _lib
from .grids import GridForm

__all__ = ["grid_tv_loss", "add_grid_tv_grad_", "grid_tv_workspace_bytes"]


def _weights(grid_weights, n: int):
    """HOST float array for the C ABI (or ``None``): the weights are call arguments like ``p``, not tensors."""
    if grid_weights is None:
        return None, 0
    if torch.is_tensor(grid_weights):
        grid_weights = grid_weights.tolist()
    w = [float(v) for v in grid_weights]
    assert len(w) == n, f"grid_weights has {len(w)} entries for {n} grids"
    return (ctypes.c_float * n)(*w), n


def grid_tv_workspace_bytes(grid_sizes) -> int:
    """Bytes of device workspace one loss evaluation of grids of these ``[B, D, H, W, C]`` sizes takes (``lp_grid_tv_workspace_bytes``;
    shapes only, no GPU)."""
    gl = GridForm.of_sizes(grid_sizes, sampler=False).abi()
    return _lib.query(_lib.lib().lp_grid_tv_workspace_bytes, ctypes.byref(gl), what="lp_grid_tv_workspace_bytes")


def _grad_args(form: GridForm, grads):
    """``(grad, grad_list, n_grad_list)`` of the C ABI for gradient tensors in ``form``."""
    if form.is_list:
        return None, (ctypes.c_void_p * len(grads))(*[t.data_ptr() for t in grads]), len(grads)
    return grads[0].data_ptr(), None, 0


class _GridTV(torch.autograd.Function):
    """loss = TV(grid tensors): forward = one sweep + the fp64 sum of its partials; backward = one gather sweep that WRITES one
    gradient per grid tensor (no concatenation, no zero-fill), scaled on the device by the upstream gradient."""

    @staticmethod
    def forward(ctx, cfg, *tensors):
        form, p, weights = cfg
        dev = tensors[0].device
        gl = form.abi(tensors)
        w, nw = _weights(weights, len(form.descs))
        L = _lib.lib()
        ws_bytes = int(L.lp_grid_tv_workspace_bytes(ctypes.byref(gl)))
        with torch.cuda.device(dev):
            workspace = torch.empty(max(ws_bytes, 8) // 8, dtype=torch.float64, device=dev)
            loss = torch.empty((), dtype=torch.float32, device=dev)
            _lib.check(L.lp_grid_tv_forward(ctypes.byref(gl), w, nw, p, loss.data_ptr(), workspace.data_ptr(), ws_bytes,
                                            _lib.current_stream(dev)), "lp_grid_tv_forward")
        ctx.cfg = cfg
        ctx.save_for_backward(*tensors)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss):
        form, p, weights = ctx.cfg
        tensors = ctx.saved_tensors
        needs = ctx.needs_input_grad[1:]
        if not any(needs):
            return (None,) * (1 + len(tensors))
        dev = tensors[0].device
        gl = form.abi(tensors)
        w, nw = _weights(weights, len(form.descs))
        g_loss = g_loss.to(device=dev, dtype=torch.float32).contiguous()
        with torch.cuda.device(dev):
            grads = [torch.empty_like(t) for t in tensors]
            _lib.check(_lib.lib().lp_grid_tv_backward(ctypes.byref(gl), w, nw, p, g_loss.data_ptr(), 1.0, *_grad_args(form, grads), 0,
                                                      _lib.current_stream(dev)), "lp_grid_tv_backward")
        return (None,) + tuple(g if need else None for g, need in zip(grads, needs))


def grid_tv_loss(grid, grid_sizes=None, p: int = 1, grid_weights: Optional[Sequence[float]] = None) -> torch.Tensor:
    """Total variation of a grid-list as a differentiable 0-dim tensor (module docstring for the definition).

    ``grid``: a *list* of ``[B, D, H, W, C]`` tensors or a flat ``[sum BDHW, C]`` tensor with ``grid_sizes``, as ``lightplane_renderer``
    takes them (anything else: ``NotImplementedError``).  ``p``: 1 or 2.  ``grid_weights``: one float per grid (default 1).
    The backward returns one gradient per list tensor.  Memory beyond the result: ``grid_tv_workspace_bytes`` in the forward, the
    gradient buffers in the backward."""
    tensors, form = GridForm.of(grid, grid_sizes, sampler=False)
    n = len(form.descs)
    weights = None if grid_weights is None else tuple(float(v) for v in (grid_weights.tolist() if torch.is_tensor(grid_weights) else grid_weights))
    assert weights is None or len(weights) == n, f"grid_weights has {len(weights)} entries for {n} grids"
    assert p in (1, 2), f"p has to be 1 (|d|) or 2 (d ** 2), got {p!r}"
    _lib.check_grids(tensors, "grid")
    return _GridTV.apply((form, int(p), weights), *tensors)


def add_grid_tv_grad_(grid, grad, weight: float = 1.0, p: int = 1, grid_sizes=None,
                      grid_weights: Optional[Sequence[float]] = None) -> torch.Tensor:
    """``grad += weight * d TV(grid) / d grid`` and the (unweighted) TV value, in ONE sweep over the grid, outside autograd.

    ``grad`` has the container shape of ``grid`` -- a list of tensors shaped like the grids (e.g. the parameters' ``.grad``), or the
    flat tensor's twin.  For a training loop::

        loss.backward()
        tv = add_grid_tv_grad_(list(grids), [g.grad for g in grids], weight=1e-3)

    Allocates nothing but the workspace (``grid_tv_workspace_bytes``) and the returned 0-dim tensor."""
    tensors, form = GridForm.of(grid, grid_sizes, sampler=False)
    if form.is_list:
        assert isinstance(grad, list) and len(grad) == len(tensors), "grad has to be a list with one tensor per grid"
        grads = tuple(grad)
    else:
        assert torch.is_tensor(grad), "grad has to be a tensor like the flat grid"
        grads = (grad,)
    for g, t in zip(grads, tensors):
        assert torch.is_tensor(g) and g.shape == t.shape and g.is_contiguous(), (
            "every gradient buffer has to be contiguous and shaped like its grid")
        assert g.data_ptr() != t.data_ptr(), "grad must not alias grid"
    w, nw = _weights(grid_weights, len(form.descs))
    _lib.check_tensors(tensors[0].device, {f"grad[{i}]": g for i, g in enumerate(grads)})
    assert p in (1, 2), f"p has to be 1 (|d|) or 2 (d ** 2), got {p!r}"
    dev = _lib.check_grids(tensors, "grid")
    gl = form.abi(tensors)
    L = _lib.lib()
    ws_bytes = int(L.lp_grid_tv_workspace_bytes(ctypes.byref(gl)))
    with torch.no_grad(), torch.cuda.device(dev):
        workspace = torch.empty(max(ws_bytes, 8) // 8, dtype=torch.float64, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        _lib.check(L.lp_grid_tv_fused(ctypes.byref(gl), w, nw, int(p), loss.data_ptr(), workspace.data_ptr(), ws_bytes, None,
                                      float(weight), *_grad_args(form, grads), _lib.current_stream(dev)), "lp_grid_tv_fused")
    return loss

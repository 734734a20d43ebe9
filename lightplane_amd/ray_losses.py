"""The distortion loss and the interlevel (proposal) loss of mip-NeRF 360 for the modular march, fused into HIP
(``csrc/lp_ray_losses.hip``; C ABI ``lp_distortion_*`` / ``lp_interlevel_*`` of ``include/lightplane_hip_losses.h``): consumers of the
weights ``composite_samples(..., return_weights=True)`` hands back.

    ray_samples -> decoder -> composite_samples (weights) -> distortion_loss
    coarse march (weights) -> importance_samples -> fine march (weights) -> interlevel_loss(fine, coarse)

Per ray, with weights ``w``, depths ``d_0 <= ... <= d_{S-1}`` and deltas:

* distortion: ``L = 2 sum_{i>j} w_i w_j (d_i - d_j) + (1/3) sum_i w_i^2 delta_i`` -- for sorted depths mip-NeRF 360's
  ``sum_ij w_i w_j |d_i - d_j|`` term, in a form that has a gradient at equal depths; computed in O(S) from scans whose terms are all
  non-negative for ``w >= 0`` (nothing cancels);
* interlevel: with the cells of ``importance_samples`` around both depth rows (edges at the ends of the span and the midpoints, in fp32)
  and ``bound_k`` the mass of every proposal cell that touches target cell ``k``, ``L = sum_k max(0, w_k - bound_k)^2 / (w_k + eps)``:
  zero where the proposal's histogram is an upper envelope of the target's.

One launch per call, one wavefront per ray; each backward is one launch that recomputes the scans, so autograd keeps the inputs only
and nothing of size ``[R, S]`` but the gradients that were asked for is allocated.  fp32, no atomics (bit-reproducible), no workspace,
no host synchronisation (graph-capturable), no double backward, no CPU path.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib

__all__ = ["distortion_loss", "interlevel_loss"]


def _call(name: str, a, stream) -> None:
    _lib.check(getattr(_lib.lib(), name)(ctypes.byref(a), stream), name)


class _Distortion(torch.autograd.Function):
    """loss [R] = distortion(weights, depths, deltas): one launch.  Backward: one launch; the three inputs are all that is saved."""

    @staticmethod
    def forward(ctx, weights, depths, deltas):
        dev = weights.device
        stream = _lib.current_stream(dev)
        weights, depths, deltas = (_lib.aligned(t.contiguous()) for t in (weights, depths, deltas))
        with torch.cuda.device(dev):
            loss = torch.empty(weights.shape[0], device=dev, dtype=torch.float32)
            a = _Distortion._args(weights, depths, deltas)
            a.loss = _lib.ptr(loss)
            _call("lp_distortion_forward", a, stream)
        ctx.save_for_backward(weights, depths, deltas)
        return loss

    @staticmethod
    def _args(weights, depths, deltas) -> _lib.LpDistortionArgs:
        a = _lib.LpDistortionArgs()
        a.n_rays, a.n_samples = weights.shape
        a.weights, a.depths, a.deltas = _lib.ptr(weights), _lib.ptr(depths), _lib.ptr(deltas)
        return a

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss):
        weights, depths, deltas = ctx.saved_tensors
        need = ctx.needs_input_grad
        if not any(need):
            return None, None, None
        dev = weights.device
        stream = _lib.current_stream(dev)
        with torch.cuda.device(dev):
            g_loss = _lib.aligned(g_loss.to(torch.float32).contiguous())
            grads = [torch.empty_like(weights) if n else None for n in need]
            a = _Distortion._args(weights, depths, deltas)
            a.grad_loss = _lib.ptr(g_loss)
            a.grad_weights, a.grad_depths, a.grad_deltas = (_lib.ptr(g) for g in grads)
            _call("lp_distortion_backward", a, stream)
        return tuple(grads)


class _Interlevel(torch.autograd.Function):
    """loss [R] = interlevel(proposal_weights | weights, depths, proposal_depths): one launch.  Backward: one launch; the four inputs
    are all that is saved."""

    @staticmethod
    def forward(ctx, eps, proposal_weights, weights, depths, proposal_depths):
        dev = weights.device
        stream = _lib.current_stream(dev)
        proposal_weights, weights, depths, proposal_depths = (_lib.aligned(t.contiguous())
                                                              for t in (proposal_weights, weights, depths, proposal_depths))
        with torch.cuda.device(dev):
            loss = torch.empty(weights.shape[0], device=dev, dtype=torch.float32)
            a = _Interlevel._args(eps, proposal_weights, weights, depths, proposal_depths)
            a.loss = _lib.ptr(loss)
            _call("lp_interlevel_forward", a, stream)
        ctx.eps = eps
        ctx.save_for_backward(proposal_weights, weights, depths, proposal_depths)
        return loss

    @staticmethod
    def _args(eps, proposal_weights, weights, depths, proposal_depths) -> _lib.LpInterlevelArgs:
        a = _lib.LpInterlevelArgs()
        a.n_rays, a.n_samples = weights.shape
        a.n_proposal, a.eps = proposal_weights.shape[1], eps
        a.weights, a.depths = _lib.ptr(weights), _lib.ptr(depths)
        a.proposal_weights, a.proposal_depths = _lib.ptr(proposal_weights), _lib.ptr(proposal_depths)
        return a

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss):
        if not ctx.needs_input_grad[1]:
            return (None,) * 5
        proposal_weights = ctx.saved_tensors[0]
        dev = proposal_weights.device
        stream = _lib.current_stream(dev)
        with torch.cuda.device(dev):
            g_loss = _lib.aligned(g_loss.to(torch.float32).contiguous())
            grad = torch.empty_like(proposal_weights)
            a = _Interlevel._args(ctx.eps, *ctx.saved_tensors)
            a.grad_loss, a.grad_proposal_weights = _lib.ptr(g_loss), _lib.ptr(grad)
            _call("lp_interlevel_backward", a, stream)
        return None, grad, None, None, None


def _check_rows(name: str, t, n: int, s: int, like: str) -> None:
    assert torch.is_tensor(t) and tuple(t.shape) == (n, s), f"{name} has to be a [{n}, {s}] tensor, as {like} is"


def distortion_loss(weights: torch.Tensor, depths: torch.Tensor, deltas: torch.Tensor) -> torch.Tensor:
    """``loss [R]``: mip-NeRF 360's distortion loss of every ray, ``2 sum_{i>j} w_i w_j (d_i - d_j) + (1/3) sum_i w_i^2 delta_i``, for
    ``weights``, ``depths`` and ``deltas`` of ``[R, S]`` each (``1 <= S <= 2048``; ``depths`` non-decreasing per ray: a contract, not
    checked) -- the weights ``composite_samples(..., return_weights=True)`` returns and the depths and deltas of the ``RaySamples`` it
    composited.  Nothing is clamped: a negative weight is a number.  Differentiable with respect to all three.

    The loss does not change when a constant is added to the depths and is homogeneous of degree 1 in ``(depths, deltas)``: mip-NeRF
    360's loss on normalised distances is ``distortion_loss(w, depths, deltas) / (far - near)``; reduce the ``[R]`` result as the
    training loop likes (usually ``.mean()``)."""
    assert torch.is_tensor(weights) and weights.ndim == 2, "weights has to be a [n_rays, n_samples] tensor"
    n, s = weights.shape
    assert 1 <= s <= _lib.LP_RAY_LOSS_MAX, f"weights has {s} samples per ray, 1 to {_lib.LP_RAY_LOSS_MAX} are supported"
    _check_rows("depths", depths, n, s, "weights")
    _check_rows("deltas", deltas, n, s, "weights")
    assert n * s < 2 ** 31, f"{n} rays x {s} samples: n_rays * n_samples has to stay below 2^31 (split the batch)"
    dev = weights.device
    _lib.check_tensors(dev, {"weights": weights, "depths": depths, "deltas": deltas})
    _lib.current_stream(dev)  # (raises for anything but a GPU: there is no CPU path)
    return _Distortion.apply(weights, depths, deltas)


def interlevel_loss(weights: torch.Tensor, depths: torch.Tensor, proposal_weights: torch.Tensor, proposal_depths: torch.Tensor, *,
                    eps: float = 1e-7) -> torch.Tensor:
    """``loss [R]``: mip-NeRF 360's interlevel loss (``lossfun_outer``) of every ray, ``sum_k max(0, w_k - bound_k)^2 / (w_k + eps)``:
    the target histogram ``weights [R, S]`` over the cells around ``depths [R, S]`` (the fine march) against ``bound_k``, the mass of
    every cell of the proposal histogram ``proposal_weights [R, P]`` over ``proposal_depths [R, P]`` (the coarse march) that touches
    target cell ``k`` (``2 <= S, P <= 2048``; both depth rows non-decreasing per ray: a contract, not checked; cells as
    ``importance_samples`` places them).  Only ``proposal_weights`` gets a gradient: ``weights``, ``depths`` and ``proposal_depths``
    are stop-gradients, as in mip-NeRF 360.  ``eps > 0``."""
    assert torch.is_tensor(weights) and weights.ndim == 2, "weights has to be a [n_rays, n_samples] tensor"
    n, s = weights.shape
    assert 2 <= s <= _lib.LP_RAY_LOSS_MAX, f"weights has {s} samples per ray, 2 to {_lib.LP_RAY_LOSS_MAX} are supported"
    _check_rows("depths", depths, n, s, "weights")
    assert torch.is_tensor(proposal_weights) and proposal_weights.ndim == 2 and proposal_weights.shape[0] == n, (
        f"proposal_weights has to be a [{n}, n_proposal] tensor: one row per row of weights")
    p = proposal_weights.shape[1]
    assert 2 <= p <= _lib.LP_RAY_LOSS_MAX, f"proposal_weights has {p} samples per ray, 2 to {_lib.LP_RAY_LOSS_MAX} are supported"
    _check_rows("proposal_depths", proposal_depths, n, p, "proposal_weights")
    eps = float(eps)
    assert math.isfinite(eps) and eps > 0.0, f"eps has to be finite and > 0, got {eps}"
    assert n * max(s, p) < 2 ** 31, f"{n} rays x {max(s, p)} samples: n_rays * max(n_samples, n_proposal) has to stay below 2^31 (split the batch)"
    dev = weights.device
    _lib.check_tensors(dev, {"weights": weights, "depths": depths, "proposal_weights": proposal_weights, "proposal_depths": proposal_depths})
    _lib.current_stream(dev)  # (raises for anything but a GPU: there is no CPU path)
    # (the target and the proposal's cells are stop-gradients: the op sees neither the fine march's graph nor the depths')
    return _Interlevel.apply(eps, proposal_weights, weights.detach(), depths.detach(), proposal_depths.detach())

"""Importance resampling for the modular march, fused into HIP (``csrc/lp_importance.hip``; C ABI ``lp_importance_samples_*`` of
``include/lightplane_hip_importance.h``): the consumer of the weights ``composite_samples(..., return_weights=True)`` hands back.

    ray_samples -> decoder -> composite_samples (weights) -> importance_samples -> decoder -> composite_samples

is NeRF's coarse -> fine pass.  Per ray, with the coarse depths ``d_0 <= ... <= d_{S-1}`` and their weights ``w``:

* edges ``e_0 = d_0``, ``e_j = (d_{j-1} + d_j) / 2``, ``e_S = d_{S-1}``: ``S`` bins, bin ``j`` the cell around coarse sample ``j`` -- every
  weight is used and no new sample leaves ``[d_0, d_{S-1}]``;
* mass ``p_j = max(w_j, 0) + pad`` (a negative or NaN weight counts as 0), ``C_{j+1} = C_j + p_j``, ``W = C_S``; a ray of all-zero weights
  gets the same mass in every bin;
* targets ``u_k = (k + xi_k) / N`` with ``xi_k = jitter[r, k]`` (the caller's ``torch.rand``: the kernel holds no RNG) or 0.5;
* ``j`` = the last bin with ``C_j <= u_k W``, ``a = clamp((u_k W - C_j) / (C_{j+1} - C_j), 0, 1)`` (0 for a zero denominator),
  ``t_k = min(max(e_j + a (e_{j+1} - e_j), e_j), e_{j+1})``: non-decreasing in ``k``, in fp32 as well;
* the result depths are the sorted union of ``d`` and ``t`` (``include_coarse``; values copied, of equal values the coarse one first) or
  ``t`` alone; ``delta'_i = depth'_i - depth'_{i-1}``, ``delta'_0 = depth'_1 - depth'_0`` (1 for a single sample);
  ``point'_i = depth'_i direction + origin``, never contracted.

The targets ascend, so the new depths come out sorted and the merge is a rank computation, not a sort: one launch, one wavefront per
ray, nothing of size ``[R, S + N]`` besides the three results.  Sample positions are a stop-gradient (as in NeRF, mip-NeRF 360 and
nerfstudio): ``depths`` and ``deltas`` of the result do not require grad, ``weights`` and the coarse ``depths`` get no gradient;
``points`` is differentiable with respect to ``rays.origins`` and ``rays.directions`` at fixed depths (pose refinement through the fine
pass).

fp32, no atomics (bit-reproducible), no workspace, no host synchronisation (graph-capturable), no double backward, no CPU path.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch

from . import _lib
from .compositing import RaySamples
from .rays import Rays

__all__ = ["importance_samples"]


def _call(name: str, a, stream) -> None:
    _lib.check(getattr(_lib.lib(), name)(ctypes.byref(a), stream), name)


class _Importance(torch.autograd.Function):
    """(points, depths, deltas) = resample(origins, directions | depths, weights, jitter): one launch, one wavefront per ray.
    Backward: one launch; ``directions`` and the result depths are all that is saved."""

    @staticmethod
    def forward(ctx, conf, origins, directions, depths, weights, jitter):
        n_importance, include_coarse, pad = conf
        dev = origins.device
        stream = _lib.current_stream(dev)
        origins, directions, depths, weights = (_lib.aligned(t.contiguous()) for t in (origins, directions, depths, weights))
        jitter = None if jitter is None else _lib.aligned(jitter.contiguous())
        n, s = depths.shape
        s_out = s + n_importance if include_coarse else n_importance
        with torch.cuda.device(dev):
            points = torch.empty(n, s_out, 3, device=dev, dtype=torch.float32)
            out_depths = torch.empty(n, s_out, device=dev, dtype=torch.float32)
            out_deltas = torch.empty(n, s_out, device=dev, dtype=torch.float32)
            a = _Importance._args(n, s, conf)
            a.origins, a.directions, a.depths, a.weights, a.jitter = (_lib.ptr(t) for t in (origins, directions, depths, weights, jitter))
            a.out_points, a.out_depths, a.out_deltas = _lib.ptr(points), _lib.ptr(out_depths), _lib.ptr(out_deltas)
            _call("lp_importance_samples_forward", a, stream)
        ctx.conf = (s, conf)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(out_depths, out_deltas)
        ctx.save_for_backward(directions, out_depths)
        return points, out_depths, out_deltas

    @staticmethod
    def _args(n: int, s: int, conf) -> _lib.LpImportanceArgs:
        a = _lib.LpImportanceArgs()
        a.n_rays, a.n_samples, a.n_importance, a.include_coarse, a.pad = n, s, conf[0], int(conf[1]), conf[2]
        return a

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_points, _g_depths, _g_deltas):
        directions, out_depths = ctx.saved_tensors
        need = ctx.needs_input_grad[1:3]
        if g_points is None or not any(need):  # (depths and deltas are not differentiable: nothing arrives through them)
            return (None,) * 6
        dev = directions.device
        stream = _lib.current_stream(dev)
        with torch.cuda.device(dev):
            g_points = _lib.aligned(g_points.to(torch.float32).contiguous())
            grads = [torch.empty_like(directions) if n else None for n in need]
            a = _Importance._args(directions.shape[0], *ctx.conf)
            a.directions, a.out_depths, a.grad_points = _lib.ptr(directions), _lib.ptr(out_depths), _lib.ptr(g_points)
            a.grad_origins, a.grad_directions = _lib.ptr(grads[0]), _lib.ptr(grads[1])
            _call("lp_importance_samples_backward", a, stream)
        return (None, *grads, None, None, None)


def importance_samples(rays: Rays, depths: torch.Tensor, weights: torch.Tensor, num_importance: int, *, include_coarse: bool = True,
                       pad: float = 1e-5, jitter: Optional[torch.Tensor] = None) -> RaySamples:
    """``RaySamples(points [R, S', 3], depths [R, S'], deltas [R, S'])``: ``num_importance = N`` new depths per ray drawn from the
    histogram that ``weights [R, S]`` (anything non-negative; negative and NaN entries count as 0) are over the coarse ``depths [R, S]``
    (non-decreasing per ray: a contract, not checked; ``2 <= S <= 2048``, ``1 <= N <= 2048``), merged into the coarse depths
    (``S' = S + N``) or, with ``include_coarse=False``, alone (``S' = N``) -- ready for the decoder and ``composite_samples`` (module
    docstring for the definition).  ``pad > 0`` is the mass every bin has besides its weight.  ``jitter``: ``None`` (the centres of the
    ``N`` strata) or ``[R, N]`` fp32 in ``[0, 1)``, the caller's ``torch.rand``.  Of ``rays`` only ``origins`` and ``directions`` are
    read.  Sample positions are a stop-gradient: ``points`` is differentiable with respect to ``rays.origins`` and ``rays.directions``,
    nothing else gets a gradient."""
    assert isinstance(rays, Rays), f"rays has to be a Rays object, got {type(rays).__name__}"
    assert torch.is_tensor(depths) and depths.ndim == 2, "depths has to be a [n_rays, n_samples] tensor"
    n, s = depths.shape
    num_importance = int(num_importance)
    assert 2 <= s <= _lib.LP_IMPORTANCE_MAX, f"depths has {s} samples per ray, 2 to {_lib.LP_IMPORTANCE_MAX} are supported"
    assert 1 <= num_importance <= _lib.LP_IMPORTANCE_MAX, f"num_importance has to be in [1, {_lib.LP_IMPORTANCE_MAX}], got {num_importance}"
    assert torch.is_tensor(weights) and tuple(weights.shape) == (n, s), f"weights has to be a [{n}, {s}] tensor, as depths is"
    pad = float(pad)
    assert math.isfinite(pad) and pad > 0.0, f"pad has to be finite and > 0, got {pad}"
    if jitter is not None:
        assert torch.is_tensor(jitter) and tuple(jitter.shape) == (n, num_importance), f"jitter has to be a [{n}, {num_importance}] tensor or None"
    for name, t in (("rays.origins", rays.origins), ("rays.directions", rays.directions)):
        assert torch.is_tensor(t) and tuple(t.shape) == (n, 3), f"{name} has to be a [{n}, 3] tensor: one ray per row of depths"
    assert n * (s + num_importance) < 2 ** 31, (
        f"{n} rays x {s + num_importance} samples: n_rays * (n_samples + num_importance) has to stay below 2^31 (split the batch)")
    dev = depths.device
    _lib.check_tensors(dev, {"rays.origins": rays.origins, "rays.directions": rays.directions, "depths": depths, "weights": weights,
                             "jitter": jitter})
    _lib.current_stream(dev)  # (raises for anything but a GPU: there is no CPU path)
    conf = (num_importance, bool(include_coarse), pad)
    # (the sample positions are a stop-gradient: the op sees neither the coarse march's graph nor the weights')
    return RaySamples(*_Importance.apply(conf, rays.origins, rays.directions, depths.detach(), weights.detach(),
                                         None if jitter is None else jitter.detach()))

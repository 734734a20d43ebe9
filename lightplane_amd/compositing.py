"""The ray march as two stand-alone ops, fused into HIP (``csrc/lp_composite.hip``; C ABI ``lp_ray_samples_*`` / ``lp_composite_*`` of
``include/lightplane_hip_samples.h``): where the Renderer places its samples, and its emission-absorption integral over per-sample
opacities and features.  With a decoder of the caller's own in between,

    ray_samples -> (sample_grid_at_points | lightplane_eval_mlp | anything) -> composite_samples

is a complete differentiable renderer: a sample lands in the grid cell the fused Renderer puts it in (the same device functions
place it), and the three results are the Renderer's.  Two things the fused Renderer does not have come with it: gradients with respect
to ray origins, directions, ``near`` and ``far`` (pose refinement), and the per-sample weights (importance resampling, distortion and
depth losses).

``ray_samples``: ``depth_i = near + linspace(0, 1, S)[i] (far - near)`` for the ``S`` regular samples and ``far / n_disp_k`` for the
``S_inf`` samples beyond ``far`` (linear in disparity down to ``disparity_at_inf``, the oracle's double arithmetic);
``delta_0 = (far - near) / (S - 1)`` (1 for ``S = 1``), ``delta_i = depth_i - depth_{i-1}``; ``point_i = depth_i direction + origin``,
never contracted -- the consumers contract.

``composite_samples``: ``od = opacity delta``, ``N_s = sum_{j<s} od_j``, ``T_s = exp(-N_s)``, ``w_s = T_s - T_{s+1}`` (computed as
``T_s (-expm1(-od_s))``: the plain difference loses five digits on transparent rays); ``ray_length = sum w depth``,
``negative_log_transmittance = N_S``, ``feature = sum w features``.  ``opacity`` is a density, already gained / activated, >= 0 by
contract and not clamped.  The backward recomputes the scan from the inputs: nothing of size ``[R, S]`` is saved besides them.

fp32, no atomics (bit-reproducible), no workspace, no host synchronisation (graph-capturable), no double backward, no CPU path.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import torch

from . import _lib
from .rays import Rays

__all__ = ["ray_samples", "composite_samples", "RaySamples"]


class RaySamples(NamedTuple):
    points: torch.Tensor  # [R, S_tot, 3]
    depths: torch.Tensor  # [R, S_tot]
    deltas: torch.Tensor  # [R, S_tot]


def _call(name: str, a, stream) -> None:
    _lib.check(getattr(_lib.lib(), name)(ctypes.byref(a), stream), name)


def _dense(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if t is None else _lib.aligned(t.to(torch.float32).contiguous())


class _RaySamples(torch.autograd.Function):
    """(points, depths, deltas) = placement(origins, directions, near, far): one launch.  Backward: one launch, one wavefront per ray."""

    @staticmethod
    def forward(ctx, march, origins, directions, near, far):
        dev = origins.device
        stream = _lib.current_stream(dev)
        origins, directions, near, far = (_lib.aligned(t.contiguous()) for t in (origins, directions, near, far))
        n, s_tot = origins.shape[0], march[0] + march[1]
        with torch.cuda.device(dev):
            points = torch.empty(n, s_tot, 3, device=dev, dtype=torch.float32)
            depths = torch.empty(n, s_tot, device=dev, dtype=torch.float32)
            deltas = torch.empty(n, s_tot, device=dev, dtype=torch.float32)
            a = _lib.LpRaySamplesArgs()
            a.rays = _lib.make_rays(directions, origins, None, near, far, None)
            a.march = _lib.make_march(march[0], march[1], False, False, march[2])
            a.points, a.depths, a.deltas = _lib.ptr(points), _lib.ptr(depths), _lib.ptr(deltas)
            _call("lp_ray_samples_forward", a, stream)
        ctx.march = march
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(origins, directions, near, far)
        return points, depths, deltas

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_points, g_depths, g_deltas):
        origins, directions, near, far = ctx.saved_tensors
        need = ctx.needs_input_grad[1:]
        if not any(need):
            return (None,) * 5
        dev = origins.device
        stream = _lib.current_stream(dev)
        ups = [_dense(g) for g in (g_points, g_depths, g_deltas)]
        with torch.cuda.device(dev):
            # (without an upstream gradient the kernel still writes the zeros asked for: every result is written entirely)
            grads = [torch.empty_like(t) if n else None for t, n in zip((origins, directions, near, far), need)]
            a = _lib.LpRaySamplesArgs()
            a.rays = _lib.make_rays(directions, origins, None, near, far, None)
            a.march = _lib.make_march(ctx.march[0], ctx.march[1], False, False, ctx.march[2])
            a.grad_points, a.grad_depths, a.grad_deltas = (_lib.ptr(g) for g in ups)
            a.grad_origins, a.grad_directions, a.grad_near, a.grad_far = (_lib.ptr(g) for g in grads)
            _call("lp_ray_samples_backward", a, stream)
        return (None, *grads)


class _Composite(torch.autograd.Function):
    """(ray_length, -log T, [feature], [weights]) = composite(opacity, features, depths, deltas): one launch, one wavefront per ray.
    Backward: one launch that recomputes the scan; only the inputs are saved."""

    @staticmethod
    def forward(ctx, return_weights: bool, opacity, features, depths, deltas):
        dev = opacity.device
        stream = _lib.current_stream(dev)
        opacity, depths, deltas = (_lib.aligned(t.contiguous()) for t in (opacity, depths, deltas))
        features = None if features is None else _lib.aligned(features.contiguous())
        n, s = opacity.shape
        c = 0 if features is None else features.shape[2]
        with torch.cuda.device(dev):
            length = torch.empty(n, device=dev, dtype=torch.float32)
            nlt = torch.empty(n, device=dev, dtype=torch.float32)
            feature = torch.empty(n, c, device=dev, dtype=torch.float32) if features is not None else None
            weights = torch.empty(n, s, device=dev, dtype=torch.float32) if return_weights else None
            a = _Composite._args(opacity, features, depths, deltas)
            a.ray_length, a.neg_log_t, a.feature, a.weights = (_lib.ptr(t) for t in (length, nlt, feature, weights))
            _call("lp_composite_forward", a, stream)
        ctx.layout = (features is not None, return_weights)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(opacity, features, depths, deltas)
        return tuple(t for t in (length, nlt, feature, weights) if t is not None)

    @staticmethod
    def _args(opacity, features, depths, deltas) -> _lib.LpCompositeArgs:
        a = _lib.LpCompositeArgs()
        a.opacity, a.features, a.depths, a.deltas = (_lib.ptr(t) for t in (opacity, features, depths, deltas))
        a.n_rays, a.n_samples = opacity.shape
        a.channels = 0 if features is None or features.shape[2] == 0 else features.shape[2]
        if a.channels == 0:
            a.features = None
        return a

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *g_outs):
        opacity, features, depths, deltas = ctx.saved_tensors
        has_feat, has_w = ctx.layout
        g_outs = list(g_outs)
        g_len, g_nlt = g_outs[0], g_outs[1]
        g_feat = g_outs[2] if has_feat else None
        g_w = g_outs[2 + has_feat] if has_w else None
        need = ctx.needs_input_grad[1:]
        if not any(need):
            return (None,) * 5
        dev = opacity.device
        stream = _lib.current_stream(dev)
        g_len, g_nlt, g_feat, g_w = (_dense(g) for g in (g_len, g_nlt, g_feat, g_w))
        with torch.cuda.device(dev):
            grads = [torch.empty_like(t) if n and t is not None else None for t, n in zip((opacity, features, depths, deltas), need)]
            a = _Composite._args(opacity, features, depths, deltas)
            a.grad_ray_length, a.grad_neg_log_t, a.grad_feature, a.grad_weights = (_lib.ptr(g) for g in (g_len, g_nlt, g_feat, g_w))
            if a.channels == 0:
                a.grad_feature = None
            a.grad_opacity, a.grad_depths, a.grad_deltas = _lib.ptr(grads[0]), _lib.ptr(grads[2]), _lib.ptr(grads[3])
            a.grad_features = _lib.ptr(grads[1]) if a.channels > 0 else None
            _call("lp_composite_backward", a, stream)
        return (None, *grads)


def ray_samples(rays: Rays, num_samples: int, num_samples_inf: int = 0, *, disparity_at_inf: float = 1e-5) -> RaySamples:
    """``RaySamples(points [R, S_tot, 3], depths [R, S_tot], deltas [R, S_tot])`` of ``rays``, ``S_tot = num_samples +
    num_samples_inf``: the samples the Renderer marches with the same three arguments (module docstring).  The points are not
    contracted.  Differentiable with respect to ``rays.origins``, ``rays.directions``, ``rays.near`` and ``rays.far``;
    ``rays.grid_idx`` and ``rays.encoding`` are not looked at."""
    assert isinstance(rays, Rays), f"rays has to be a Rays object, got {type(rays).__name__}"
    num_samples, num_samples_inf = int(num_samples), int(num_samples_inf)
    assert num_samples >= 1, f"num_samples has to be >= 1, got {num_samples}"
    assert num_samples_inf >= 0, f"num_samples_inf has to be >= 0, got {num_samples_inf}"
    dev = rays.directions.device
    _lib.check_tensors(dev, {"rays.origins": rays.origins, "rays.directions": rays.directions, "rays.near": rays.near,
                             "rays.far": rays.far})
    n = rays.directions.shape[0]
    assert n * (num_samples + num_samples_inf) < 2 ** 31, (
        f"{n} rays x {num_samples + num_samples_inf} samples: n_rays * samples has to stay below 2^31 (split the batch)")
    _lib.current_stream(dev)  # (raises for anything but a GPU: there is no CPU path)
    march = (num_samples, num_samples_inf, float(disparity_at_inf))
    return RaySamples(*_RaySamples.apply(march, rays.origins, rays.directions, rays.near, rays.far))


def composite_samples(opacity, features, depths, deltas, *, return_weights: bool = False):
    """``(ray_length_render [R], negative_log_transmittance [R], feature_render [R, C])`` -- the Renderer's results -- from per-sample
    ``opacity [R, S]`` (a density >= 0, already gained / activated; not clamped), ``features [R, S, C]`` (or ``None``: then
    ``feature_render`` is ``None``), ``depths [R, S]`` and ``deltas [R, S]`` (module docstring for the definition); with
    ``return_weights=True`` a fourth result, the compositing weights ``w [R, S]``.  ``0 <= C <= 128``, any value.  Differentiable with
    respect to all four inputs (and through ``weights``)."""
    assert torch.is_tensor(opacity) and opacity.ndim == 2, "opacity has to be a [n_rays, n_samples] tensor"
    n, s = opacity.shape
    assert s >= 1, "opacity has to have one sample per ray at least"
    for name, t in (("depths", depths), ("deltas", deltas)):
        assert torch.is_tensor(t) and tuple(t.shape) == (n, s), f"{name} has to be a [{n}, {s}] tensor, as opacity is"
    if features is not None:
        assert torch.is_tensor(features) and features.ndim == 3 and tuple(features.shape[:2]) == (n, s), (
            f"features has to be a [{n}, {s}, C] tensor or None")
        assert features.shape[2] <= _lib.LP_MAX_WIDTH, f"features has {features.shape[2]} channels, at most {_lib.LP_MAX_WIDTH} are supported"
    assert n * s < 2 ** 31, f"{n} rays x {s} samples: n_rays * n_samples has to stay below 2^31 (split the batch)"
    dev = opacity.device
    _lib.check_tensors(dev, {"opacity": opacity, "features": features, "depths": depths, "deltas": deltas})
    _lib.current_stream(dev)  # (raises for anything but a GPU: there is no CPU path)
    outs = list(_Composite.apply(bool(return_weights), opacity, features, depths, deltas))
    if features is None:
        outs.insert(2, None)
    return tuple(outs)

"""Space-time plane encoding of 3-D points with a timestamp (the K-Planes field representation; HexPlane and, without the time planes,
the Hadamard tri-plane are the same arithmetic), fused into HIP (``csrc/lp_kplanes.hip``; C ABI ``lp_kplanes_forward`` /
``lp_kplanes_backward_planes`` / ``lp_kplanes_backward_points``).  It plugs into the march in pieces,
``ray_samples -> kplanes_encode -> a decoder of the caller's -> composite_samples``, without a change to any other op.

A **layout** (``kplanes_layout``) is computed here; the kernels read it as tables.  There are ``S = len(resolutions)`` scales; scale
``s`` has ``n_s`` vertices on each of x, y and z.  ``time_resolution=None`` is the *static* variant, ``P = 3`` planes per scale in the
order xy, xz, yz; an int or a length-``S`` tuple is the *dynamic* variant, ``P = 6``: xt, yt, zt follow, with ``m_s`` vertices on t.
A plane over the axes ``(u, v)`` has ``n_u n_v`` vertices and vertex ``(i_u, i_v)`` is row ``i_u + n_u i_v``; all planes of all scales
sit back to back (``offsets[s][j]`` is the first row of plane ``j`` of scale ``s``) in one ``[B, rows, C]`` fp32 tensor for ``B``
scenes.

Encoding of point ``p`` of row ``r`` (batch element ``ray_grid_idx[r]``, clamped) at time ``tau`` (``times[r]`` or ``times[r, n]``, in
``[-1, 1]``): ``q = p`` or, with ``contract_coords``, the Renderer's contraction (into ``[-1, 1]^3``); with
``mask_out_of_bounds_samples`` a point whose ``q`` leaves ``[-1, 1]^3`` has all features and all gradients exactly 0 (time never
masks).  On an axis of ``n`` vertices ``x = clamp(fma(q, (n - 1) / 2, (n - 1) / 2), 0, n - 1)``, ``i = min(floor(x), n - 2)``,
``f = x - i`` -- the same on every plane that holds the axis; ``tau`` goes through the same map with ``m_s``.  With ``v_j`` the bilinear
value of plane ``j`` at its two coordinates (4 vertices, weights ``(1 - f | f)``), ``out[r, n, s C + c] = prod_j v_j[c]``: an
elementwise product, scales concatenated scale-major, no normalisation.  Gradients go to ``planes`` (fp32 atomics; rows no point touches
stay exactly 0) and to ``points`` (stored, bit-reproducible, zero on a clamped axis); ``times`` and ``ray_grid_idx`` get none.  No
derivative divides by a plane value.  No host synchronisation (graph-capturable); there is no double backward and no CPU path.

**The decoder on it, in one launch.**  ``kplanes_eval_mlp`` / ``kplanes_eval_mlp_opacity_only`` (``csrc/lp_kplanes_points.hip``; C ABI
``lp_kplanes_points_forward`` / ``lp_kplanes_points_backward``) evaluate the library's decoder on this encoding: ``t = ReLU(trunk(feat))``
(``ReLU(feat)`` without trunk layers), ``opacity = gain softplus(opacity MLP(t)) occ``, ``colour = sigmoid(colour MLP(t +
rays_encoding[r]))[:color_chn] occ``, ``occ`` the scaffold's nearest-neighbour value at ``q`` (1 without one) -- the decoder of
``hash_grid_eval_mlp``.  The features ``[n_rays, n_pts, S C]`` and their gradient never reach memory: ``ray_samples -> kplanes_eval_mlp
-> composite_samples`` is a differentiable renderer of a time-dependent field.  One autograd function that keeps its inputs only;
gradients go to ``planes``, ``decoder_params.mlp_params``, ``rays_encoding`` and ``points``, a gradient nobody asks for is not computed,
and without an upstream colour gradient the colour head is not evaluated (its parameters get exactly 0).

**The render along rays, in one launch.**  ``kplanes_render_samples`` (``csrc/lp_kplanes_render.hip``; C ABI
``lp_kplanes_render_forward`` / ``lp_kplanes_render_backward``) is that chain fused: it forms every sample's point
``depth * direction + origin`` in registers, decodes it as ``kplanes_eval_mlp`` does and composites as ``composite_samples`` does
(``w_s = exp(-sum_{j<s} opacity_j delta_j) (-expm1(-opacity_s delta_s))``), one wavefront per ray, so no ``[R, S]`` points, opacity or
colour tensor exists in either direction -- it means what ``hash_grid_render_samples`` means, on the only field here that reads time.
One autograd function that keeps its inputs and one ``chunk_nlt [R, ceil(S / 64)]`` buffer; gradients go to ``planes``,
``decoder_params.mlp_params`` and ``rays.encoding`` (stored, bit-reproducible); ``depths``, ``deltas``, the ray origins and directions
and ``times`` get none (the modular chain differentiates with respect to the first four).
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Sequence, Tuple, Union

import torch

from . import _lib
from .params import DecoderParams, int_list_of
from .rays import Rays
from .render_samples import chunks

__all__ = ["KPlanesLayout", "kplanes_layout", "init_kplanes", "kplanes_encode", "kplanes_eval_mlp", "kplanes_eval_mlp_opacity_only",
           "kplanes_render_samples"]


class KPlanesLayout(NamedTuple):
    n_scales: int
    n_planes: int
    channels: int
    spatial: Tuple[int, ...]
    temporal: Tuple[int, ...]
    offsets: Tuple[Tuple[int, ...], ...]
    rows: int
    out_channels: int


def kplanes_layout(resolutions: Sequence[int] = (64, 128, 256, 512), time_resolution: Union[None, int, Sequence[int]] = None,
                   channels: int = 32) -> KPlanesLayout:
    """The layout of a plane field (module docstring): vertices per axis and the first row of every plane of every scale."""
    spatial = tuple(int(n) for n in resolutions)
    S, C, top = len(spatial), int(channels), _lib.LP_KPLANES_MAX_RESOLUTION
    if not 1 <= S <= _lib.LP_KPLANES_MAX_SCALES:
        raise ValueError(f"{S} resolutions: the number of scales has to be in [1, {_lib.LP_KPLANES_MAX_SCALES}]")
    if C not in (4, 8, 16, 32, 64):
        raise ValueError(f"channels {C} is not one of 4, 8, 16, 32, 64")
    if S * C > _lib.LP_MAX_WIDTH:
        raise ValueError(f"scales x channels = {S * C} channels > {_lib.LP_MAX_WIDTH}")
    if time_resolution is None:
        temporal = ()
    elif isinstance(time_resolution, int):
        temporal = (int(time_resolution),) * S
    else:
        temporal = tuple(int(m) for m in time_resolution)
        if len(temporal) != S:
            raise ValueError(f"time_resolution has {len(temporal)} entries for {S} scales")
    for n in spatial + temporal:
        if not 2 <= n <= top:
            raise ValueError(f"resolution {n} outside [2, {top}]")
    P = 6 if temporal else 3
    offsets, row = [], 0
    for s in range(S):
        sizes = [spatial[s] * spatial[s]] * 3 + ([spatial[s] * temporal[s]] * 3 if temporal else [])
        offsets.append(tuple(row + sum(sizes[:j]) for j in range(P)))
        row += sum(sizes)
    return KPlanesLayout(S, P, C, spatial, temporal, tuple(offsets), row, S * C)


def init_kplanes(layout: KPlanesLayout, batch: int = 1, *, low: float = 0.1, high: float = 0.5, device=None,
                 generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """A ``[batch, layout.rows, C]`` fp32 tensor: the space planes uniform in ``[low, high]``, the space-time planes 1 (the usual
    initialisation: a fresh dynamic field equals its static part)."""
    t = torch.rand(int(batch), layout.rows, layout.channels, device=device, dtype=torch.float32, generator=generator)
    t.mul_(float(high) - float(low)).add_(float(low))
    if layout.n_planes == 6:
        for s in range(layout.n_scales):
            t[:, layout.offsets[s][3]:layout.offsets[s][5] + layout.spatial[s] * layout.temporal[s]] = 1.0
    return t


class _Cfg(NamedTuple):
    layout: KPlanesLayout
    mask: bool
    contract: bool


def _args(cfg: _Cfg, points, times, grid_idx, batch: int, a=None):
    """the layout, the points, the timestamps and the flags in a fresh ``LpKPlanesArgs`` (or in ``a``, which has the same fields)"""
    lay = cfg.layout
    a = _lib.LpKPlanesArgs() if a is None else a
    a.points, a.grid_idx, a.times = _lib.ptr(points), _lib.ptr(grid_idx), _lib.ptr(times)
    a.time_per_point = int(times is not None and times.ndim == 2)
    a.n_rays, a.n_pts = points.shape[0], points.shape[1]
    a.batch, a.rows = batch, lay.rows
    a.channels, a.n_scales, a.n_planes = lay.channels, lay.n_scales, lay.n_planes
    for s in range(lay.n_scales):
        a.spatial[s] = lay.spatial[s]
        a.temporal[s] = lay.temporal[s] if lay.temporal else 0
        for j in range(lay.n_planes):
            a.offset[s][j] = lay.offsets[s][j]
    a.mask_out_of_bounds, a.contract_coords = int(cfg.mask), int(cfg.contract)
    return a


def _call(name: str, a, stream) -> None:
    _lib.check(getattr(_lib.lib(), name)(ctypes.byref(a), stream), name)


class _KPlanesEncode(torch.autograd.Function):
    """features = encode(points, times, planes): one launch, no atomics.  Backward: the run-merged atomic scatter into a zeroed twin of
    the planes (when the planes ask) and the stored point gradient (when ``points`` asks) -- a kernel nobody asks for does not run."""

    @staticmethod
    def forward(ctx, cfg: _Cfg, points, times, planes, grid_idx):
        dev = points.device
        stream = _lib.current_stream(dev)
        points, planes = _lib.aligned(points.contiguous()), _lib.aligned(planes.contiguous(), grid=True)
        times = None if times is None else _lib.aligned(times.contiguous())
        with torch.cuda.device(dev):
            out = torch.empty(points.shape[0], points.shape[1], cfg.layout.out_channels, device=dev, dtype=torch.float32)
            a = _args(cfg, points, times, grid_idx, planes.shape[0])
            a.planes, a.out_features = _lib.ptr(planes), _lib.ptr(out)
            if out.numel():  # (an empty batch has no tensors to point at)
                _call("lp_kplanes_forward", a, stream)
        ctx.cfg = cfg
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(points, times, planes, grid_idx)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        cfg: _Cfg = ctx.cfg
        points, times, planes, grid_idx = ctx.saved_tensors
        need = ctx.needs_input_grad
        if g_out is None or not (need[1] or need[3]):
            return None, None, None, None, None
        dev = points.device
        stream = _lib.current_stream(dev)
        g_out = _lib.aligned(g_out.to(torch.float32).contiguous())
        d_points, d_planes = None, None
        with torch.cuda.device(dev):
            a = _args(cfg, points, times, grid_idx, planes.shape[0])
            a.planes, a.grad_features = _lib.ptr(planes), _lib.ptr(g_out)
            if need[1]:
                d_points = torch.empty_like(points)
                a.grad_points = _lib.ptr(d_points)
                if g_out.numel():
                    _call("lp_kplanes_backward_points", a, stream)
            if need[3]:
                d_planes = torch.zeros_like(planes)
                a.grad_planes = _lib.ptr(d_planes)
                if g_out.numel():
                    _call("lp_kplanes_backward_planes", a, stream)
        return None, d_points, None, d_planes, None


def _check_inputs(points, times, planes, ray_grid_idx, layout) -> None:
    """what the op asks of its points, times, planes, ray_grid_idx and layout (before any device is touched)"""
    if not isinstance(layout, KPlanesLayout):
        raise ValueError("layout has to be the KPlanesLayout of kplanes_layout()")
    assert torch.is_tensor(points) and points.ndim == 3 and points.shape[-1] == 3, "points has to be a [n_rays, n_pts, 3] tensor"
    _check_field(points.shape[0], points.shape[1], times, planes, ray_grid_idx, layout)


def _check_field(n_rays: int, n_pts: int, times, planes, ray_grid_idx, layout) -> None:
    """... of the times, planes and ray_grid_idx of ``n_rays`` rows of ``n_pts`` points (or samples)"""
    assert torch.is_tensor(ray_grid_idx) and tuple(ray_grid_idx.shape) == (n_rays,), f"ray_grid_idx has to be a [{n_rays}] tensor"
    assert not ray_grid_idx.is_floating_point() and not ray_grid_idx.is_complex() and ray_grid_idx.dtype != torch.bool, (
        "ray_grid_idx has to have an integer dtype")
    assert n_rays * n_pts < 1 << 31, f"points: {n_rays} x {n_pts} has to stay below 2^31"
    if layout.n_planes == 3:
        if times is not None:
            raise ValueError("times has to be None for a static layout (time_resolution=None)")
    else:
        if not torch.is_tensor(times):
            raise ValueError("times has to be a tensor for a dynamic layout (one timestamp per row, or one per point)")
        assert tuple(times.shape) in ((n_rays,), (n_rays, n_pts)), f"times has to be a [{n_rays}] or a [{n_rays}, {n_pts}] tensor"
        if times.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("times requires a gradient, and kplanes_encode produces none for the timestamps: pass times.detach()")
    if not torch.is_tensor(planes) or planes.ndim != 3 or planes.shape[0] < 1 or tuple(planes.shape[1:]) != (layout.rows, layout.channels):
        shape = tuple(planes.shape) if torch.is_tensor(planes) else type(planes).__name__
        raise ValueError(f"planes has to be a [B, {layout.rows}, {layout.channels}] tensor for this layout (got {shape})")


def kplanes_encode(points, times, planes, ray_grid_idx, layout: KPlanesLayout, *, mask_out_of_bounds_samples: bool = False,
                   contract_coords: bool = False) -> torch.Tensor:
    """``features [n_rays, n_pts, S C]``: the plane encoding (module docstring) of ``points [n_rays, n_pts, 3]`` at ``times``
    (``[n_rays]`` or ``[n_rays, n_pts]``, read as it is -- no expanded copy; ``None`` for a static layout) with the
    ``planes [B, layout.rows, C]`` of ``init_kplanes``; ``ray_grid_idx [n_rays]`` (any integer dtype): the scene of each row's points.
    Differentiable with respect to ``planes`` and ``points``; ``times`` must not require a gradient (``.detach()`` it)."""
    _check_inputs(points, times, planes, ray_grid_idx, layout)
    _lib.check_tensors(points.device, {"points": points, "times": times, "planes": planes}, {"ray_grid_idx": ray_grid_idx})
    _lib.current_stream(points.device)  # (raises for anything but a GPU: there is no CPU path)
    grid_idx = _lib.int32_index(ray_grid_idx)
    cfg = _Cfg(layout, bool(mask_out_of_bounds_samples), bool(contract_coords))
    return _KPlanesEncode.apply(cfg, points, None if times is None else times.detach(), planes, grid_idx)


class _EvalCfg(NamedTuple):
    planes: _Cfg
    dims_t: tuple
    dims_o: tuple
    dims_c: tuple
    color_chn: int
    gain: float
    opacity_only: bool


def _eval_args(cfg: _EvalCfg, points, times, planes, mlp_params, encoding, grid_idx, scaffold, with_color: bool) -> _lib.LpKPlanesPointsArgs:
    a = _args(cfg.planes, points, times, grid_idx, planes.shape[0], _lib.LpKPlanesPointsArgs())
    a.planes = _lib.ptr(planes)
    a.mlp_params, a.n_mlp_params = _lib.ptr(mlp_params), mlp_params.numel()
    _lib.make_decoder(a, cfg.dims_t, cfg.dims_o, cfg.dims_c)
    a.color_chn, a.gain = cfg.color_chn, cfg.gain
    if with_color:
        a.encoding, a.encoding_dim = _lib.ptr(encoding), encoding.shape[1]
    if scaffold is not None:
        a.scaffold = _lib.ptr(scaffold)
        a.scaffold_shape = _lib.LpGrid(*[int(v) for v in scaffold.shape], 0, None)
    return a


class _KPlanesEval(torch.autograd.Function):
    """(opacity[, colour]) = decoder(encode(points, times, planes)): one forward launch; the backward is one launch that recomputes
    every point and fills the gradients ``needs_input_grad`` asks for (a gradient nobody asks for is a NULL pointer: its work is
    skipped; without an upstream gradient for the colour, the colour head is not evaluated)."""

    @staticmethod
    def forward(ctx, cfg: _EvalCfg, points, times, planes, mlp_params, encoding, grid_idx, scaffold):
        dev = points.device
        stream = _lib.current_stream(dev)
        points, planes = _lib.aligned(points.contiguous()), _lib.aligned(planes.contiguous(), grid=True)
        times = None if times is None else _lib.aligned(times.contiguous())
        mlp_params = _lib.aligned(mlp_params.contiguous())
        encoding = None if encoding is None else _lib.aligned(encoding.contiguous())
        n_rays, n_pts = points.shape[0], points.shape[1]
        with torch.cuda.device(dev):
            opacity = torch.empty(n_rays, n_pts, device=dev, dtype=torch.float32)
            color = None if cfg.opacity_only else torch.empty(n_rays, n_pts, cfg.color_chn, device=dev, dtype=torch.float32)
            a = _eval_args(cfg, points, times, planes, mlp_params, encoding, grid_idx, scaffold, not cfg.opacity_only)
            a.opacity_out, a.color_out = _lib.ptr(opacity), _lib.ptr(color)
            if opacity.numel():  # (an empty batch has no tensors to point at)
                _call("lp_kplanes_points_forward", a, stream)
        ctx.cfg = cfg
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(points, times, planes, mlp_params, encoding, grid_idx, scaffold)
        return opacity if cfg.opacity_only else (opacity, color)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_opacity, g_color=None):
        cfg: _EvalCfg = ctx.cfg
        points, times, planes, mlp_params, encoding, grid_idx, scaffold = ctx.saved_tensors
        need = ctx.needs_input_grad
        if (g_opacity is None and g_color is None) or not any(need):
            return (None,) * 8
        dev = points.device
        stream = _lib.current_stream(dev)
        with_color = g_color is not None and not cfg.opacity_only
        g_opacity = None if g_opacity is None else _lib.aligned(g_opacity.to(torch.float32).contiguous())
        g_color = _lib.aligned(g_color.to(torch.float32).contiguous()) if with_color else None
        with torch.cuda.device(dev):
            d_points = torch.empty_like(points) if need[1] else None
            d_planes = torch.zeros_like(planes) if need[3] else None
            d_params = torch.zeros_like(mlp_params) if need[4] else None
            d_enc = torch.zeros_like(encoding) if (need[5] and encoding is not None) else None
            a = _eval_args(cfg, points, times, planes, mlp_params, encoding, grid_idx, scaffold, with_color)
            a.grad_opacity, a.grad_color = _lib.ptr(g_opacity), _lib.ptr(g_color)
            a.grad_points, a.grad_planes, a.grad_mlp_params = _lib.ptr(d_points), _lib.ptr(d_planes), _lib.ptr(d_params)
            a.grad_encoding = _lib.ptr(d_enc) if with_color else None
            if points.numel():
                _call("lp_kplanes_points_backward", a, stream)
        return None, d_points, None, d_planes, d_params, d_enc, None, None


def _eval(points, times, planes, ray_grid_idx, layout, decoder_params: DecoderParams, rays_encoding, gain, mask, contract, scaffold,
          opacity_only: bool):
    _check_inputs(points, times, planes, ray_grid_idx, layout)
    n_rays = points.shape[0]
    dims_t, dims_o, dims_c = (tuple(int_list_of(v)) for v in (decoder_params.n_hidden_trunk, decoder_params.n_hidden_opacity,
                                                              decoder_params.n_hidden_color))
    width = dims_t[0] if len(dims_t) > 1 else dims_o[0]
    if width != layout.out_channels:
        raise ValueError(f"the decoder reads {width} features, the layout has n_scales x channels = {layout.out_channels}")
    if opacity_only:
        rays_encoding = None
    else:
        assert torch.is_tensor(rays_encoding) and tuple(rays_encoding.shape) == (n_rays, dims_c[0]), (
            f"rays_encoding has to be a [{n_rays}, {dims_c[0]}] tensor (the colour head's input width)")
    mlp_params = decoder_params.mlp_params
    assert mlp_params.ndim == 1, "decoder_params.mlp_params has to be the flat parameter vector"
    if scaffold is not None:
        assert torch.is_tensor(scaffold) and scaffold.ndim == 4, "scaffold has to be a [B, D, H, W] tensor"
    dev = points.device
    _lib.check_tensors(dev, {"points": points, "times": times, "planes": planes, "decoder_params.mlp_params": mlp_params,
                             "rays_encoding": rays_encoding, "scaffold": scaffold}, {"ray_grid_idx": ray_grid_idx})
    _lib.current_stream(dev)  # (raises for anything but a GPU: there is no CPU path)
    grid_idx = _lib.int32_index(ray_grid_idx)
    scaffold = None if scaffold is None else _lib.aligned(scaffold.detach().contiguous())
    cfg = _EvalCfg(_Cfg(layout, bool(mask), bool(contract)), dims_t, dims_o, dims_c, int(decoder_params.color_chn), float(gain),
                   opacity_only)
    return _KPlanesEval.apply(cfg, points, None if times is None else times.detach(), planes, mlp_params, rays_encoding, grid_idx,
                              scaffold)


def kplanes_eval_mlp(points, times, planes, ray_grid_idx, layout: KPlanesLayout, decoder_params: DecoderParams, rays_encoding,
                     gain: float, *, mask_out_of_bounds_samples: bool = False, contract_coords: bool = False,
                     scaffold: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(opacity [n_rays, n_pts], colour [n_rays, n_pts, color_chn])`` of the decoder on the plane encoding of
    ``points [n_rays, n_pts, 3]`` at ``times`` (module docstring), in one launch.  ``times``, ``planes``, ``ray_grid_idx``, ``layout``:
    as ``kplanes_encode``; ``decoder_params``: a decoder whose trunk (without trunk layers: whose heads) reads ``layout.out_channels``
    features; ``rays_encoding [n_rays, E]``: added to the colour head's input; ``scaffold``: ``[B, D, H, W]`` occupancy or ``None``.
    Differentiable with respect to ``planes``, ``decoder_params.mlp_params``, ``rays_encoding`` and ``points``."""
    return _eval(points, times, planes, ray_grid_idx, layout, decoder_params, rays_encoding, gain, mask_out_of_bounds_samples,
                 contract_coords, scaffold, False)


def kplanes_eval_mlp_opacity_only(points, times, planes, ray_grid_idx, layout: KPlanesLayout, decoder_params: DecoderParams, gain: float,
                                  *, mask_out_of_bounds_samples: bool = False, contract_coords: bool = False,
                                  scaffold: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``opacity [n_rays, n_pts]`` alone: the opacity of ``kplanes_eval_mlp``, bit for bit, without the colour head -- there is no
    encoding, and the colour MLP's parameters are never read (they get exactly zero gradient)."""
    return _eval(points, times, planes, ray_grid_idx, layout, decoder_params, None, gain, mask_out_of_bounds_samples, contract_coords,
                 scaffold, True)


class _RenderCfg(NamedTuple):
    planes: _Cfg
    dims_t: tuple
    dims_o: tuple
    dims_c: tuple
    color_chn: int
    gain: float
    return_weights: bool
    with_color: bool


def _render_args(cfg: _RenderCfg, origins, directions, grid_idx, times, depths, deltas, scaffold, planes, mlp_params, encoding,
                 with_color: bool) -> _lib.LpKPlanesRenderArgs:
    lay = cfg.planes.layout
    a = _lib.LpKPlanesRenderArgs()
    a.planes, a.batch, a.rows = _lib.ptr(planes), planes.shape[0], lay.rows
    a.channels, a.n_scales, a.n_planes = lay.channels, lay.n_scales, lay.n_planes
    for s in range(lay.n_scales):
        a.spatial[s] = lay.spatial[s]
        a.temporal[s] = lay.temporal[s] if lay.temporal else 0
        for j in range(lay.n_planes):
            a.offset[s][j] = lay.offsets[s][j]
    a.times, a.time_per_sample = _lib.ptr(times), int(times is not None and times.ndim == 2)
    a.mask_out_of_bounds, a.contract_coords = int(cfg.planes.mask), int(cfg.planes.contract)
    a.mlp_params, a.n_mlp_params = _lib.ptr(mlp_params), mlp_params.numel()
    _lib.make_decoder(a, cfg.dims_t, cfg.dims_o, cfg.dims_c)
    a.color_chn, a.gain = cfg.color_chn, cfg.gain
    a.origins, a.directions, a.grid_idx = _lib.ptr(origins), _lib.ptr(directions), _lib.ptr(grid_idx)
    if with_color:
        a.encoding, a.encoding_dim = _lib.ptr(encoding), encoding.shape[1]
    a.n_rays, a.n_samples = depths.shape
    a.depths, a.deltas = _lib.ptr(depths), _lib.ptr(deltas)
    if scaffold is not None:
        a.scaffold = _lib.ptr(scaffold)
        a.scaffold_shape = _lib.LpGrid(*[int(v) for v in scaffold.shape], 0, None)
    return a


class _KPlanesRender(torch.autograd.Function):
    """(ray_length, -log T[, feature][, weights]) = render(depths, deltas; planes, times, decoder, encoding): one forward launch; the
    backward is one launch that recomputes every sample and fills the gradients ``needs_input_grad`` asks for (a gradient nobody asks
    for is a NULL pointer: its work is skipped; a result nobody differentiated is a NULL upstream gradient).  Kept for it: the inputs
    and ``chunk_nlt [R, ceil(S / 64)]``."""

    @staticmethod
    def forward(ctx, cfg: _RenderCfg, origins, directions, grid_idx, times, depths, deltas, scaffold, planes, mlp_params, encoding):
        dev = depths.device
        stream = _lib.current_stream(dev)
        origins, directions, depths, deltas, mlp_params = (
            _lib.aligned(t.contiguous()) for t in (origins, directions, depths, deltas, mlp_params))
        times = None if times is None else _lib.aligned(times.contiguous())
        planes = _lib.aligned(planes.contiguous(), grid=True)
        encoding = _lib.aligned(encoding.contiguous()) if cfg.with_color else None
        n, s = depths.shape
        with torch.cuda.device(dev):
            length = torch.empty(n, device=dev, dtype=torch.float32)
            nlt = torch.empty(n, device=dev, dtype=torch.float32)
            feature = torch.empty(n, cfg.color_chn, device=dev, dtype=torch.float32) if cfg.with_color else None
            weights = torch.empty(n, s, device=dev, dtype=torch.float32) if cfg.return_weights else None
            chunk_nlt = torch.empty(n, chunks(s), device=dev, dtype=torch.float32)
            a = _render_args(cfg, origins, directions, grid_idx, times, depths, deltas, scaffold, planes, mlp_params, encoding,
                             cfg.with_color)
            a.ray_length, a.neg_log_t, a.feature, a.weights = (_lib.ptr(t) for t in (length, nlt, feature, weights))
            a.chunk_nlt = _lib.ptr(chunk_nlt)
            if n:  # (an empty batch has no tensors to point at)
                _call("lp_kplanes_render_forward", a, stream)
        ctx.cfg = cfg
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(origins, directions, grid_idx, times, depths, deltas, scaffold, planes, mlp_params, encoding, chunk_nlt)
        return tuple(t for t in (length, nlt, feature, weights) if t is not None)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_len, g_nlt, *rest):
        cfg: _RenderCfg = ctx.cfg
        origins, directions, grid_idx, times, depths, deltas, scaffold, planes, mlp_params, encoding, chunk_nlt = ctx.saved_tensors
        need = ctx.needs_input_grad
        rest = list(rest)
        g_feat = rest.pop(0) if cfg.with_color else None
        g_w = rest.pop(0) if cfg.return_weights else None
        ups = (g_len, g_nlt, g_feat, g_w)
        if all(g is None for g in ups) or not any(need):
            return (None,) * 11
        dev = depths.device
        stream = _lib.current_stream(dev)
        g_len, g_nlt, g_feat, g_w = (None if g is None else _lib.aligned(g.to(torch.float32).contiguous()) for g in ups)
        with_color = g_feat is not None
        with torch.cuda.device(dev):
            d_planes = torch.zeros_like(planes) if need[8] else None
            d_params = torch.zeros_like(mlp_params) if need[9] else None
            d_enc = torch.empty_like(encoding) if (need[10] and encoding is not None) else None  # (written entirely)
            a = _render_args(cfg, origins, directions, grid_idx, times, depths, deltas, scaffold, planes, mlp_params, encoding, with_color)
            a.chunk_nlt = _lib.ptr(chunk_nlt)
            a.grad_ray_length, a.grad_neg_log_t, a.grad_feature, a.grad_weights = (_lib.ptr(g) for g in (g_len, g_nlt, g_feat, g_w))
            a.grad_planes, a.grad_mlp_params, a.grad_encoding = _lib.ptr(d_planes), _lib.ptr(d_params), _lib.ptr(d_enc)
            if d_enc is not None:
                a.encoding_dim = encoding.shape[1]  # (without an upstream for the feature the kernel stores zeros: the row length)
            if depths.shape[0]:
                _call("lp_kplanes_render_backward", a, stream)
        return None, None, None, None, None, None, None, None, d_planes, d_params, d_enc


def kplanes_render_samples(rays: Rays, times, depths: torch.Tensor, deltas: torch.Tensor, planes: torch.Tensor, layout: KPlanesLayout,
                           decoder_params: DecoderParams, *, gain: float = 1.0, mask_out_of_bounds_samples: bool = False,
                           contract_coords: bool = False, scaffold: Optional[torch.Tensor] = None, return_weights: bool = False,
                           with_color: bool = True):
    """``(ray_length_render [R], negative_log_transmittance [R], feature_render [R, color_chn])`` of ``rays`` marched through the plane
    field ``planes`` / ``layout`` / ``decoder_params`` at the caller's ``depths [R, S]`` with the interval lengths ``deltas [R, S]``
    (fp32: ``RaySamples.depths`` / ``.deltas`` of ``ray_samples`` or ``importance_samples``) at ``times`` (``[R]`` or ``[R, S]``, read
    as it is -- no expanded copy; ``None`` for a static layout); with ``return_weights=True`` a fourth result, the compositing weights
    ``w [R, S]``.  Any ``S >= 1`` with ``R * S < 2^31``.

    Of ``rays`` the op reads ``origins``, ``directions``, ``grid_idx`` and ``encoding``.  ``planes``, ``layout``, ``decoder_params``,
    ``gain``, ``mask_out_of_bounds_samples``, ``contract_coords`` and ``scaffold`` mean what they mean in ``kplanes_eval_mlp``.
    ``with_color=False`` (the coarse / proposal pass that only wants weights): ``feature_render`` is ``None``, the colour MLP and
    ``rays.encoding`` are never read in either direction, and the other results are the same bit for bit.  Differentiable with
    respect to ``planes``, ``decoder_params.mlp_params`` and ``rays.encoding``; ``depths``, ``deltas``, ``rays.origins``,
    ``rays.directions`` and ``times`` must not require a gradient (module docstring)."""
    assert isinstance(rays, Rays), f"rays has to be a Rays object, got {type(rays).__name__}"
    assert torch.is_tensor(depths) and depths.ndim == 2, "depths has to be a [n_rays, n_samples] tensor"
    n, s = depths.shape
    assert s >= 1, "depths has to have one sample per ray at least"
    assert torch.is_tensor(deltas) and tuple(deltas.shape) == (n, s), f"deltas has to be a [{n}, {s}] tensor, as depths is"
    assert n * s < 2 ** 31, f"depths: {n} rays x {s} samples: n_rays * n_samples has to stay below 2^31 (split the batch)"
    for name, t in (("rays.origins", rays.origins), ("rays.directions", rays.directions)):
        assert torch.is_tensor(t) and tuple(t.shape) == (n, 3), f"{name} has to be a [{n}, 3] tensor: one ray per row of depths"
    if torch.is_grad_enabled():
        for name, t in (("depths", depths), ("deltas", deltas), ("rays.origins", rays.origins), ("rays.directions", rays.directions),
                        ("times", times)):
            if torch.is_tensor(t) and t.requires_grad:
                raise NotImplementedError(
                    f"{name} requires a gradient, and kplanes_render_samples produces none for depths, deltas, ray origins and "
                    f"directions and times: pass {name}.detach(), or use the modular chain (ray_samples / importance_samples -> "
                    "kplanes_eval_mlp -> composite_samples), which differentiates with respect to the first four")
    if not isinstance(layout, KPlanesLayout):
        raise ValueError("layout has to be the KPlanesLayout of kplanes_layout()")
    _check_field(n, s, times, planes, rays.grid_idx, layout)
    dims_t, dims_o, dims_c = (tuple(int_list_of(v)) for v in (decoder_params.n_hidden_trunk, decoder_params.n_hidden_opacity,
                                                              decoder_params.n_hidden_color))
    width = dims_t[0] if len(dims_t) > 1 else dims_o[0]
    if width != layout.out_channels:
        raise ValueError(f"the decoder reads {width} features, the layout has n_scales x channels = {layout.out_channels}")
    encoding = rays.encoding if with_color else None
    if with_color:
        assert torch.is_tensor(encoding) and tuple(encoding.shape) == (n, dims_c[0]), (
            f"rays.encoding has to be a [{n}, {dims_c[0]}] tensor (the colour head's input width)")
    mlp_params = decoder_params.mlp_params
    assert mlp_params.ndim == 1, "decoder_params.mlp_params has to be the flat parameter vector"
    if scaffold is not None:
        assert torch.is_tensor(scaffold) and scaffold.ndim == 4, "scaffold has to be a [B, D, H, W] tensor"
    dev = depths.device
    _lib.check_tensors(dev, {"depths": depths, "deltas": deltas, "rays.origins": rays.origins, "rays.directions": rays.directions,
                             "times": times, "planes": planes, "decoder_params.mlp_params": mlp_params, "rays.encoding": encoding,
                             "scaffold": scaffold}, {"rays.grid_idx": rays.grid_idx})
    _lib.current_stream(dev)  # (raises for anything but a GPU: there is no CPU path)
    grid_idx = _lib.int32_index(rays.grid_idx)
    scaffold = None if scaffold is None else _lib.aligned(scaffold.detach().contiguous())
    cfg = _RenderCfg(_Cfg(layout, bool(mask_out_of_bounds_samples), bool(contract_coords)), dims_t, dims_o, dims_c,
                     int(decoder_params.color_chn), float(gain), bool(return_weights), bool(with_color))
    out = _KPlanesRender.apply(cfg, rays.origins.detach(), rays.directions.detach(), grid_idx, None if times is None else times.detach(),
                               depths.detach(), deltas.detach(), scaffold, planes, mlp_params, encoding)
    if with_color:
        return out
    return (out[0], out[1], None) + tuple(out[2:])

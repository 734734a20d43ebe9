"""Multiresolution hash-grid encoding of 3-D points (the Instant-NGP field representation), fused into HIP (``csrc/lp_hash_grid.hip``;
C ABI ``lp_hash_grid_forward`` / ``lp_hash_grid_backward_table`` / ``lp_hash_grid_backward_points``).  It plugs into the march in
pieces, ``ray_samples -> hash_grid_encode -> a decoder of the caller's -> composite_samples``, without a change to any other op.

A **layout** (``hash_grid_layout``) is computed here in Python doubles; the kernels read it as tables.  With ``L`` levels of ``F``
features, ``T = 1 << log2_table_size``, ``N_0 = base_resolution`` and, for ``L > 1``,
``N_l = floor(N_0 (N_max / N_0)^(l / (L - 1)) + 1e-6)`` (the last level forced to ``N_max = finest_resolution``), level ``l`` has a lattice
of ``S_l = N_l + 1`` vertices per axis.  It is *dense* when ``S_l^3 <= T`` -- entry ``ix + S_l (iy + S_l iz)``, ``S_l^3`` entries rounded
up to a multiple of 8 -- and *hashed* otherwise: ``T`` entries, entry ``(ix ^ iy * 2654435761 ^ iz * 805459861) & (T - 1)`` in wrapping
uint32 arithmetic.  ``offsets`` are the running sum of the sizes, ``entries`` their total; the table is one ``[B, entries, F]`` fp32
tensor for ``B`` scenes, as a grid-list batch.

Encoding of point ``p`` of row ``r`` (batch element ``ray_grid_idx[r]``, clamped): ``q = p`` or, with ``contract_coords``, the
Renderer's contraction (into ``[-1, 1]^3``); with ``mask_out_of_bounds_samples`` a point whose ``q`` leaves ``[-1, 1]^3`` has all features
and all gradients exactly 0.  Per axis ``x = clamp((q + 1) / 2, 0, 1) N_l``, ``i = min(floor(x), N_l - 1)``, ``f = x - i``; the 8 corners
``i + {0, 1}`` carry the trilinear weights ``(1 - f | f)``, and ``out[r, n, l F + c] = sum_k w_k table[b, offset_l + index_l(corner_k), c]``
(level-major channels; colliding corners add).  Gradients go to ``table`` and to ``points`` (zero on a clamped axis), none through
``ray_grid_idx``.  fp32 coordinates limit a level's interpolation weights to about ``N_l * 2^-24`` cells.  The table gradient is
accumulated with fp32 atomics (values and point gradients are bit-reproducible).  No host synchronisation (graph-capturable); there is
no double backward and no CPU path.

``hash_grid_eval_mlp`` / ``hash_grid_eval_mlp_opacity_only`` (``csrc/lp_hash_points.hip``; C ABI ``lp_hash_points_forward`` /
``lp_hash_points_backward``) evaluate the decoder of ``lightplane_eval_mlp`` on this encoding in ONE launch, so that the features
``[n_rays, n_pts, L F]`` and their gradient never reach memory: ``ray_samples -> hash_grid_eval_mlp -> composite_samples`` is a
hash-grid renderer.  With ``feat`` the encoding above::

    t = relu(trunk(feat)) (relu(feat) without trunk layers);  raw = opacity_mlp(t);  craw = color_mlp(t + rays_encoding[r])
    opacity = gain * softplus(raw) * occ;   colour = sigmoid(craw)[:color_chn] * occ;   occ = scaffold at q (1 without a scaffold)

Gradients go to ``table``, ``decoder_params.mlp_params``, ``rays_encoding`` and ``points``; the backward recomputes every point and
reads nothing the forward wrote.

``hash_grid_render_samples`` (``csrc/lp_hash_render.hip``; C ABI ``lp_hash_render_forward`` / ``lp_hash_render_backward``) is that
renderer in ONE launch, ``ray_samples | importance_samples -> hash_grid_render_samples``: sample ``s`` of ray ``r`` is evaluated at
``depths[r, s] * direction + origin`` (formed in registers), decoded as ``hash_grid_eval_mlp`` decodes a point and composited as
``composite_samples`` does.  No ``[R, S]`` tensor exists but the weights the caller asks for; autograd keeps the inputs and one
``[R, ceil(S / 64)]`` buffer.  Gradients go to ``table``, ``decoder_params.mlp_params`` and ``rays.encoding``; ``depths``, ``deltas``,
``rays.origins`` and ``rays.directions`` get NONE (``NotImplementedError`` if one of them requires one: ``.detach()`` it, or use the
chain).  The forward and the encoding gradient are bit-reproducible; table and parameter gradients are accumulated with atomics.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib
from .params import DecoderParams, int_list_of
from .rays import Rays
from .render_samples import chunks

__all__ = ["HashGridLayout", "hash_grid_layout", "init_hash_grid", "hash_grid_encode", "hash_grid_eval_mlp",
           "hash_grid_eval_mlp_opacity_only", "hash_grid_render_samples"]


class HashGridLayout(NamedTuple):
    n_levels: int
    features_per_level: int
    log2_table_size: int
    resolutions: Tuple[int, ...]
    offsets: Tuple[int, ...]
    sizes: Tuple[int, ...]
    hashed: Tuple[bool, ...]
    entries: int
    channels: int


def hash_grid_layout(n_levels: int = 16, features_per_level: int = 2, log2_table_size: int = 19, base_resolution: int = 16,
                     finest_resolution: int = 2048) -> HashGridLayout:
    """The layout of a hash grid (module docstring): resolutions, offsets, sizes and dense / hashed per level."""
    L, F, n_min, n_max = int(n_levels), int(features_per_level), int(base_resolution), int(finest_resolution)
    if not 1 <= L <= _lib.LP_HASH_MAX_LEVELS:
        raise ValueError(f"n_levels {L} outside [1, {_lib.LP_HASH_MAX_LEVELS}]")
    if F not in (1, 2, 4, 8):
        raise ValueError(f"features_per_level {F} is not one of 1, 2, 4, 8")
    if L * F > _lib.LP_MAX_WIDTH:
        raise ValueError(f"n_levels x features_per_level = {L * F} channels > {_lib.LP_MAX_WIDTH}")
    if not 3 <= int(log2_table_size) <= 24:
        raise ValueError(f"log2_table_size {log2_table_size} outside [3, 24]")
    if not 1 <= n_min <= n_max <= 65536:
        raise ValueError(f"1 <= base_resolution {n_min} <= finest_resolution {n_max} <= 65536 does not hold")
    T = 1 << int(log2_table_size)
    res = [n_min if l == 0 else int(float(n_min) * (float(n_max) / float(n_min)) ** (l / (L - 1)) + 1e-6) for l in range(L)]
    if L > 1:
        res[-1] = n_max
    hashed = tuple((n + 1) ** 3 > T for n in res)
    sizes = tuple(T if h else ((n + 1) ** 3 + 7) // 8 * 8 for n, h in zip(res, hashed))
    offsets = tuple(sum(sizes[:l]) for l in range(L))
    return HashGridLayout(L, F, int(log2_table_size), tuple(res), offsets, sizes, hashed, sum(sizes), L * F)


def init_hash_grid(layout: HashGridLayout, batch: int = 1, *, scale: float = 1e-4, device=None,
                   generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """A ``[batch, layout.entries, F]`` fp32 table, uniform in ``[-scale, scale]`` (the usual initialisation of the encoding)."""
    t = torch.rand(int(batch), layout.entries, layout.features_per_level, device=device, dtype=torch.float32, generator=generator)
    return t.mul_(2.0 * scale).sub_(scale)


class _Cfg(NamedTuple):
    layout: HashGridLayout
    mask: bool
    contract: bool


def _args(cfg: _Cfg, points, grid_idx, batch: int, a=None):
    """the layout, the points and the flags in ``a`` (a fresh ``LpHashGridArgs`` by default)"""
    lay = cfg.layout
    a = _lib.LpHashGridArgs() if a is None else a
    a.points, a.grid_idx = _lib.ptr(points), _lib.ptr(grid_idx)
    a.n_rays, a.n_pts = points.shape[0], points.shape[1]
    a.batch, a.entries = batch, lay.entries
    a.features_per_level, a.n_levels = lay.features_per_level, lay.n_levels
    for l in range(lay.n_levels):
        a.resolution[l], a.offset[l], a.size[l], a.hashed[l] = lay.resolutions[l], lay.offsets[l], lay.sizes[l], int(lay.hashed[l])
    a.mask_out_of_bounds, a.contract_coords = int(cfg.mask), int(cfg.contract)
    return a


def _call(name: str, a: _lib.LpHashGridArgs, stream) -> None:
    _lib.check(getattr(_lib.lib(), name)(ctypes.byref(a), stream), name)


class _HashGridEncode(torch.autograd.Function):
    """features = encode(points, table): one launch, no atomics.  Backward: the atomic scatter of the upstream gradient into a zeroed
    twin of the table (when the table asks) and the stored point gradient (when ``points`` asks) -- a kernel nobody asks for does not
    run."""

    @staticmethod
    def forward(ctx, cfg: _Cfg, points, table, grid_idx):
        dev = points.device
        stream = _lib.current_stream(dev)
        points, table = _lib.aligned(points.contiguous()), _lib.aligned(table.contiguous(), grid=True)
        with torch.cuda.device(dev):
            out = torch.empty(points.shape[0], points.shape[1], cfg.layout.channels, device=dev, dtype=torch.float32)
            a = _args(cfg, points, grid_idx, table.shape[0])
            a.table, a.out_features = _lib.ptr(table), _lib.ptr(out)
            if out.numel():  # (an empty batch has no tensors to point at)
                _call("lp_hash_grid_forward", a, stream)
        ctx.cfg = cfg
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(points, table, grid_idx)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        cfg: _Cfg = ctx.cfg
        points, table, grid_idx = ctx.saved_tensors
        need = ctx.needs_input_grad
        if g_out is None or not (need[1] or need[2]):
            return None, None, None, None
        dev = points.device
        stream = _lib.current_stream(dev)
        g_out = _lib.aligned(g_out.to(torch.float32).contiguous())
        d_points, d_table = None, None
        with torch.cuda.device(dev):
            a = _args(cfg, points, grid_idx, table.shape[0])
            a.table, a.grad_features = _lib.ptr(table), _lib.ptr(g_out)
            if need[1]:
                d_points = torch.empty_like(points)
                a.grad_points = _lib.ptr(d_points)
                if g_out.numel():
                    _call("lp_hash_grid_backward_points", a, stream)
            if need[2]:
                d_table = torch.zeros_like(table)
                a.grad_table = _lib.ptr(d_table)
                if g_out.numel():
                    _call("lp_hash_grid_backward_table", a, stream)
        return None, d_points, d_table, None


def _check_inputs(points, table, ray_grid_idx, layout) -> None:
    """what every front-end of this module asks of its points, table, ray_grid_idx and layout (before any device is touched)"""
    assert torch.is_tensor(points) and points.ndim == 3 and points.shape[-1] == 3, "points has to be a [n_rays, n_pts, 3] tensor"
    n_rays = points.shape[0]
    assert torch.is_tensor(ray_grid_idx) and tuple(ray_grid_idx.shape) == (n_rays,), f"ray_grid_idx has to be a [{n_rays}] tensor"
    assert not ray_grid_idx.is_floating_point() and not ray_grid_idx.is_complex() and ray_grid_idx.dtype != torch.bool, (
        "ray_grid_idx has to have an integer dtype")
    assert points.shape[0] * points.shape[1] < 1 << 31, f"points: {points.shape[0]} x {points.shape[1]} has to stay below 2^31"
    _check_table(table, layout)


def _check_table(table, layout) -> None:
    if not isinstance(layout, HashGridLayout):
        raise ValueError("layout has to be the HashGridLayout of hash_grid_layout()")
    if not torch.is_tensor(table) or table.ndim != 3 or table.shape[0] < 1 or tuple(table.shape[1:]) != (layout.entries, layout.features_per_level):
        shape = tuple(table.shape) if torch.is_tensor(table) else type(table).__name__
        raise ValueError(f"table has to be a [B, {layout.entries}, {layout.features_per_level}] tensor for this layout (got {shape})")


def hash_grid_encode(points, table, ray_grid_idx, layout: HashGridLayout, *, mask_out_of_bounds_samples: bool = False,
                     contract_coords: bool = False) -> torch.Tensor:
    """``features [n_rays, n_pts, L F]``: the hash-grid encoding (module docstring) of ``points [n_rays, n_pts, 3]`` with the
    ``table [B, layout.entries, F]`` of ``init_hash_grid``; ``ray_grid_idx [n_rays]`` (any integer dtype): the scene of each row's
    points.  Differentiable with respect to ``table`` and ``points``."""
    _check_inputs(points, table, ray_grid_idx, layout)
    _lib.check_tensors(points.device, {"points": points, "table": table}, {"ray_grid_idx": ray_grid_idx})
    _lib.current_stream(points.device)  # (raises for anything but a GPU: there is no CPU path)
    grid_idx = _lib.int32_index(ray_grid_idx)
    cfg = _Cfg(layout, bool(mask_out_of_bounds_samples), bool(contract_coords))
    return _HashGridEncode.apply(cfg, points, table, grid_idx)


class _EvalCfg(NamedTuple):
    hash: _Cfg
    dims_t: tuple
    dims_o: tuple
    dims_c: tuple
    color_chn: int
    gain: float
    opacity_only: bool


def _eval_args(cfg: _EvalCfg, points, table, mlp_params, encoding, grid_idx, scaffold, with_color: bool) -> _lib.LpHashPointsArgs:
    a = _args(cfg.hash, points, grid_idx, table.shape[0], _lib.LpHashPointsArgs())
    a.table = _lib.ptr(table)
    a.mlp_params, a.n_mlp_params = _lib.ptr(mlp_params), mlp_params.numel()
    _lib.make_decoder(a, cfg.dims_t, cfg.dims_o, cfg.dims_c)
    a.color_chn, a.gain = cfg.color_chn, cfg.gain
    if with_color:
        a.encoding, a.encoding_dim = _lib.ptr(encoding), encoding.shape[1]
    if scaffold is not None:
        a.scaffold = _lib.ptr(scaffold)
        a.scaffold_shape = _lib.LpGrid(*[int(v) for v in scaffold.shape], 0, None)
    return a


class _HashGridEval(torch.autograd.Function):
    """(opacity[, colour]) = decoder(encode(points, table)): one forward launch; the backward is one launch that recomputes every
    point and fills the gradients ``needs_input_grad`` asks for (a gradient nobody asks for is a NULL pointer: its work is skipped;
    without an upstream gradient for the colour, the colour head is not evaluated)."""

    @staticmethod
    def forward(ctx, cfg: _EvalCfg, points, table, mlp_params, encoding, grid_idx, scaffold):
        dev = points.device
        stream = _lib.current_stream(dev)
        points, table = _lib.aligned(points.contiguous()), _lib.aligned(table.contiguous(), grid=True)
        mlp_params = _lib.aligned(mlp_params.contiguous())
        encoding = None if encoding is None else _lib.aligned(encoding.contiguous())
        n_rays, n_pts = points.shape[0], points.shape[1]
        with torch.cuda.device(dev):
            opacity = torch.empty(n_rays, n_pts, device=dev, dtype=torch.float32)
            color = None if cfg.opacity_only else torch.empty(n_rays, n_pts, cfg.color_chn, device=dev, dtype=torch.float32)
            a = _eval_args(cfg, points, table, mlp_params, encoding, grid_idx, scaffold, not cfg.opacity_only)
            a.opacity_out, a.color_out = _lib.ptr(opacity), _lib.ptr(color)
            if opacity.numel():  # (an empty batch has no tensors to point at)
                _call("lp_hash_points_forward", a, stream)
        ctx.cfg = cfg
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(points, table, mlp_params, encoding, grid_idx, scaffold)
        return opacity if cfg.opacity_only else (opacity, color)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_opacity, g_color=None):
        cfg: _EvalCfg = ctx.cfg
        points, table, mlp_params, encoding, grid_idx, scaffold = ctx.saved_tensors
        need = ctx.needs_input_grad
        if (g_opacity is None and g_color is None) or not any(need):
            return (None,) * 7
        dev = points.device
        stream = _lib.current_stream(dev)
        with_color = g_color is not None and not cfg.opacity_only
        g_opacity = None if g_opacity is None else _lib.aligned(g_opacity.to(torch.float32).contiguous())
        g_color = _lib.aligned(g_color.to(torch.float32).contiguous()) if with_color else None
        with torch.cuda.device(dev):
            d_points = torch.empty_like(points) if need[1] else None
            d_table = torch.zeros_like(table) if need[2] else None
            d_params = torch.zeros_like(mlp_params) if need[3] else None
            d_enc = torch.zeros_like(encoding) if (need[4] and encoding is not None) else None
            a = _eval_args(cfg, points, table, mlp_params, encoding, grid_idx, scaffold, with_color)
            a.grad_opacity, a.grad_color = _lib.ptr(g_opacity), _lib.ptr(g_color)
            a.grad_points, a.grad_table, a.grad_mlp_params = _lib.ptr(d_points), _lib.ptr(d_table), _lib.ptr(d_params)
            a.grad_encoding = _lib.ptr(d_enc) if with_color else None
            if points.numel():
                _call("lp_hash_points_backward", a, stream)
        return None, d_points, d_table, d_params, d_enc, None, None


def _eval(points, table, ray_grid_idx, layout, decoder_params: DecoderParams, rays_encoding, gain, mask, contract, scaffold,
          opacity_only: bool):
    _check_inputs(points, table, ray_grid_idx, layout)
    n_rays = points.shape[0]
    dims_t, dims_o, dims_c = (tuple(int_list_of(v)) for v in (decoder_params.n_hidden_trunk, decoder_params.n_hidden_opacity,
                                                              decoder_params.n_hidden_color))
    width = dims_t[0] if len(dims_t) > 1 else dims_o[0]
    if width != layout.channels:
        raise ValueError(f"the decoder reads {width} features, the layout has n_levels x features_per_level = {layout.channels}")
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
    _lib.check_tensors(dev, {"points": points, "table": table, "decoder_params.mlp_params": mlp_params, "rays_encoding": rays_encoding,
                             "scaffold": scaffold}, {"ray_grid_idx": ray_grid_idx})
    _lib.current_stream(dev)  # (raises for anything but a GPU: there is no CPU path)
    grid_idx = _lib.int32_index(ray_grid_idx)
    scaffold = None if scaffold is None else _lib.aligned(scaffold.detach().contiguous())
    cfg = _EvalCfg(_Cfg(layout, bool(mask), bool(contract)), dims_t, dims_o, dims_c, int(decoder_params.color_chn), float(gain),
                   opacity_only)
    return _HashGridEval.apply(cfg, points, table, mlp_params, rays_encoding, grid_idx, scaffold)


def hash_grid_eval_mlp(points, table, ray_grid_idx, layout: HashGridLayout, decoder_params: DecoderParams, rays_encoding, gain: float, *,
                       mask_out_of_bounds_samples: bool = False, contract_coords: bool = False,
                       scaffold: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(opacity [n_rays, n_pts], colour [n_rays, n_pts, color_chn])`` of the decoder on the hash-grid encoding of
    ``points [n_rays, n_pts, 3]`` (module docstring), in one launch.  ``table``, ``ray_grid_idx``, ``layout``: as ``hash_grid_encode``;
    ``decoder_params``: a decoder whose trunk (without trunk layers: whose heads) reads ``layout.channels`` features;
    ``rays_encoding [n_rays, E]``: added to the colour head's input; ``scaffold``: ``[B, D, H, W]`` occupancy or ``None``.
    Differentiable with respect to ``table``, ``decoder_params.mlp_params``, ``rays_encoding`` and ``points``."""
    return _eval(points, table, ray_grid_idx, layout, decoder_params, rays_encoding, gain, mask_out_of_bounds_samples, contract_coords,
                 scaffold, False)


def hash_grid_eval_mlp_opacity_only(points, table, ray_grid_idx, layout: HashGridLayout, decoder_params: DecoderParams, gain: float, *,
                                    mask_out_of_bounds_samples: bool = False, contract_coords: bool = False,
                                    scaffold: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``opacity [n_rays, n_pts]`` alone: the opacity of ``hash_grid_eval_mlp``, bit for bit, without the colour head -- there is no
    encoding, and the colour MLP's parameters are never read (they get exactly zero gradient)."""
    return _eval(points, table, ray_grid_idx, layout, decoder_params, None, gain, mask_out_of_bounds_samples, contract_coords, scaffold, True)


class _RenderCfg(NamedTuple):
    hash: _Cfg
    dims_t: tuple
    dims_o: tuple
    dims_c: tuple
    color_chn: int
    gain: float
    return_weights: bool
    with_color: bool


def _render_args(cfg: _RenderCfg, origins, directions, grid_idx, depths, deltas, scaffold, table, mlp_params, encoding,
                 with_color: bool) -> _lib.LpHashRenderArgs:
    lay = cfg.hash.layout
    a = _lib.LpHashRenderArgs()
    a.table, a.batch, a.entries = _lib.ptr(table), table.shape[0], lay.entries
    a.features_per_level, a.n_levels = lay.features_per_level, lay.n_levels
    for l in range(lay.n_levels):
        a.resolution[l], a.offset[l], a.size[l], a.hashed[l] = lay.resolutions[l], lay.offsets[l], lay.sizes[l], int(lay.hashed[l])
    a.mask_out_of_bounds, a.contract_coords = int(cfg.hash.mask), int(cfg.hash.contract)
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


class _HashGridRender(torch.autograd.Function):
    """(ray_length, -log T[, feature][, weights]) = render(depths, deltas; table, decoder, encoding): one forward launch; the backward
    is one launch that recomputes every sample and fills the gradients ``needs_input_grad`` asks for (a gradient nobody asks for is a
    NULL pointer: its work is skipped; a result nobody differentiated is a NULL upstream gradient).  Kept for it: the inputs and
    ``chunk_nlt [R, ceil(S / 64)]``."""

    @staticmethod
    def forward(ctx, cfg: _RenderCfg, origins, directions, grid_idx, depths, deltas, scaffold, table, mlp_params, encoding):
        dev = depths.device
        stream = _lib.current_stream(dev)
        origins, directions, depths, deltas, mlp_params = (
            _lib.aligned(t.contiguous()) for t in (origins, directions, depths, deltas, mlp_params))
        table = _lib.aligned(table.contiguous(), grid=True)
        encoding = _lib.aligned(encoding.contiguous()) if cfg.with_color else None
        n, s = depths.shape
        with torch.cuda.device(dev):
            length = torch.empty(n, device=dev, dtype=torch.float32)
            nlt = torch.empty(n, device=dev, dtype=torch.float32)
            feature = torch.empty(n, cfg.color_chn, device=dev, dtype=torch.float32) if cfg.with_color else None
            weights = torch.empty(n, s, device=dev, dtype=torch.float32) if cfg.return_weights else None
            chunk_nlt = torch.empty(n, chunks(s), device=dev, dtype=torch.float32)
            a = _render_args(cfg, origins, directions, grid_idx, depths, deltas, scaffold, table, mlp_params, encoding, cfg.with_color)
            a.ray_length, a.neg_log_t, a.feature, a.weights = (_lib.ptr(t) for t in (length, nlt, feature, weights))
            a.chunk_nlt = _lib.ptr(chunk_nlt)
            if n:  # (an empty batch has no tensors to point at)
                _lib.check(_lib.lib().lp_hash_render_forward(ctypes.byref(a), stream), "lp_hash_render_forward")
        ctx.cfg = cfg
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(origins, directions, grid_idx, depths, deltas, scaffold, table, mlp_params, encoding, chunk_nlt)
        return tuple(t for t in (length, nlt, feature, weights) if t is not None)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_len, g_nlt, *rest):
        cfg: _RenderCfg = ctx.cfg
        origins, directions, grid_idx, depths, deltas, scaffold, table, mlp_params, encoding, chunk_nlt = ctx.saved_tensors
        need = ctx.needs_input_grad
        rest = list(rest)
        g_feat = rest.pop(0) if cfg.with_color else None
        g_w = rest.pop(0) if cfg.return_weights else None
        ups = (g_len, g_nlt, g_feat, g_w)
        if all(g is None for g in ups) or not any(need):
            return (None,) * 10
        dev = depths.device
        stream = _lib.current_stream(dev)
        g_len, g_nlt, g_feat, g_w = (None if g is None else _lib.aligned(g.to(torch.float32).contiguous()) for g in ups)
        with_color = g_feat is not None
        with torch.cuda.device(dev):
            d_table = torch.zeros_like(table) if need[7] else None
            d_params = torch.zeros_like(mlp_params) if need[8] else None
            d_enc = torch.empty_like(encoding) if (need[9] and encoding is not None) else None  # (written entirely)
            a = _render_args(cfg, origins, directions, grid_idx, depths, deltas, scaffold, table, mlp_params, encoding, with_color)
            a.chunk_nlt = _lib.ptr(chunk_nlt)
            a.grad_ray_length, a.grad_neg_log_t, a.grad_feature, a.grad_weights = (_lib.ptr(g) for g in (g_len, g_nlt, g_feat, g_w))
            a.grad_table, a.grad_mlp_params, a.grad_encoding = _lib.ptr(d_table), _lib.ptr(d_params), _lib.ptr(d_enc)
            if d_enc is not None:
                a.encoding_dim = encoding.shape[1]  # (without an upstream for the feature the kernel stores zeros: the row length)
            if depths.shape[0]:
                _lib.check(_lib.lib().lp_hash_render_backward(ctypes.byref(a), stream), "lp_hash_render_backward")
        return None, None, None, None, None, None, None, d_table, d_params, d_enc


def hash_grid_render_samples(rays: Rays, depths: torch.Tensor, deltas: torch.Tensor, table: torch.Tensor, layout: HashGridLayout,
                             decoder_params: DecoderParams, *, gain: float = 1.0, mask_out_of_bounds_samples: bool = False,
                             contract_coords: bool = False, scaffold: Optional[torch.Tensor] = None, return_weights: bool = False,
                             with_color: bool = True):
    """``(ray_length_render [R], negative_log_transmittance [R], feature_render [R, color_chn])`` of ``rays`` marched through the
    hash-grid field ``table`` / ``layout`` / ``decoder_params`` at the caller's ``depths [R, S]`` with the interval lengths
    ``deltas [R, S]`` (fp32: ``RaySamples.depths`` / ``.deltas`` of ``ray_samples`` or ``importance_samples``); with
    ``return_weights=True`` a fourth result, the compositing weights ``w [R, S]``.  Any ``S >= 1`` with ``R * S < 2^31``.

    Of ``rays`` the op reads ``origins``, ``directions``, ``grid_idx`` and ``encoding``.  ``table``, ``layout``, ``decoder_params``,
    ``gain``, ``mask_out_of_bounds_samples``, ``contract_coords`` and ``scaffold`` mean what they mean in ``hash_grid_eval_mlp``.
    ``with_color=False`` (the coarse / proposal pass that only wants weights): ``feature_render`` is ``None``, the colour MLP and
    ``rays.encoding`` are never read in either direction, and the other results are the same bit for bit.  Differentiable with
    respect to ``table``, ``decoder_params.mlp_params`` and ``rays.encoding``; ``depths``, ``deltas``, ``rays.origins`` and
    ``rays.directions`` must not require a gradient (module docstring)."""
    assert isinstance(rays, Rays), f"rays has to be a Rays object, got {type(rays).__name__}"
    assert torch.is_tensor(depths) and depths.ndim == 2, "depths has to be a [n_rays, n_samples] tensor"
    n, s = depths.shape
    assert s >= 1, "depths has to have one sample per ray at least"
    assert torch.is_tensor(deltas) and tuple(deltas.shape) == (n, s), f"deltas has to be a [{n}, {s}] tensor, as depths is"
    assert n * s < 2 ** 31, f"depths: {n} rays x {s} samples: n_rays * n_samples has to stay below 2^31 (split the batch)"
    for name, t in (("rays.origins", rays.origins), ("rays.directions", rays.directions)):
        assert torch.is_tensor(t) and tuple(t.shape) == (n, 3), f"{name} has to be a [{n}, 3] tensor: one ray per row of depths"
    assert torch.is_tensor(rays.grid_idx) and tuple(rays.grid_idx.shape) == (n,), f"rays.grid_idx has to be a [{n}] tensor"
    _check_table(table, layout)
    dims_t, dims_o, dims_c = (tuple(int_list_of(v)) for v in (decoder_params.n_hidden_trunk, decoder_params.n_hidden_opacity,
                                                              decoder_params.n_hidden_color))
    width = dims_t[0] if len(dims_t) > 1 else dims_o[0]
    if width != layout.channels:
        raise ValueError(f"the decoder reads {width} features, the layout has n_levels x features_per_level = {layout.channels}")
    encoding = rays.encoding if with_color else None
    if with_color:
        assert torch.is_tensor(encoding) and tuple(encoding.shape) == (n, dims_c[0]), (
            f"rays.encoding has to be a [{n}, {dims_c[0]}] tensor (the colour head's input width)")
    if torch.is_grad_enabled():
        for name, t in (("depths", depths), ("deltas", deltas), ("rays.origins", rays.origins), ("rays.directions", rays.directions)):
            if t.requires_grad:
                raise NotImplementedError(
                    f"{name} requires a gradient, and hash_grid_render_samples produces none for depths, deltas, ray origins and "
                    f"directions: pass {name}.detach(), or use the modular chain (ray_samples / importance_samples -> "
                    "hash_grid_eval_mlp -> composite_samples), which differentiates with respect to them")
    mlp_params = decoder_params.mlp_params
    assert mlp_params.ndim == 1, "decoder_params.mlp_params has to be the flat parameter vector"
    if scaffold is not None:
        assert torch.is_tensor(scaffold) and scaffold.ndim == 4, "scaffold has to be a [B, D, H, W] tensor"
    dev = depths.device
    _lib.check_tensors(dev, {"depths": depths, "deltas": deltas, "rays.origins": rays.origins, "rays.directions": rays.directions,
                             "table": table, "decoder_params.mlp_params": mlp_params, "rays.encoding": encoding, "scaffold": scaffold},
                       {"rays.grid_idx": rays.grid_idx})
    _lib.current_stream(dev)  # (raises for anything but a GPU: there is no CPU path)
    grid_idx = _lib.int32_index(rays.grid_idx)
    scaffold = None if scaffold is None else _lib.aligned(scaffold.detach().contiguous())
    cfg = _RenderCfg(_Cfg(layout, bool(mask_out_of_bounds_samples), bool(contract_coords)), dims_t, dims_o, dims_c,
                     int(decoder_params.color_chn), float(gain), bool(return_weights), bool(with_color))
    out = _HashGridRender.apply(cfg, rays.origins.detach(), rays.directions.detach(), grid_idx, depths.detach(), deltas.detach(), scaffold,
                                table, mlp_params, encoding)
    if with_color:
        return out
    return (out[0], out[1], None) + tuple(out[2:])

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
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib

__all__ = ["HashGridLayout", "hash_grid_layout", "init_hash_grid", "hash_grid_encode"]


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


def _args(cfg: _Cfg, points, grid_idx, batch: int) -> _lib.LpHashGridArgs:
    lay = cfg.layout
    a = _lib.LpHashGridArgs()
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


def hash_grid_encode(points, table, ray_grid_idx, layout: HashGridLayout, *, mask_out_of_bounds_samples: bool = False,
                     contract_coords: bool = False) -> torch.Tensor:
    """``features [n_rays, n_pts, L F]``: the hash-grid encoding (module docstring) of ``points [n_rays, n_pts, 3]`` with the
    ``table [B, layout.entries, F]`` of ``init_hash_grid``; ``ray_grid_idx [n_rays]`` (any integer dtype): the scene of each row's
    points.  Differentiable with respect to ``table`` and ``points``."""
    assert torch.is_tensor(points) and points.ndim == 3 and points.shape[-1] == 3, "points has to be a [n_rays, n_pts, 3] tensor"
    n_rays = points.shape[0]
    assert torch.is_tensor(ray_grid_idx) and tuple(ray_grid_idx.shape) == (n_rays,), f"ray_grid_idx has to be a [{n_rays}] tensor"
    assert not ray_grid_idx.is_floating_point() and not ray_grid_idx.is_complex() and ray_grid_idx.dtype != torch.bool, (
        "ray_grid_idx has to have an integer dtype")
    assert points.shape[0] * points.shape[1] < 1 << 31, f"points: {points.shape[0]} x {points.shape[1]} has to stay below 2^31"
    if not isinstance(layout, HashGridLayout):
        raise ValueError("layout has to be the HashGridLayout of hash_grid_layout()")
    if not torch.is_tensor(table) or table.ndim != 3 or table.shape[0] < 1 or tuple(table.shape[1:]) != (layout.entries, layout.features_per_level):
        shape = tuple(table.shape) if torch.is_tensor(table) else type(table).__name__
        raise ValueError(f"table has to be a [B, {layout.entries}, {layout.features_per_level}] tensor for this layout (got {shape})")
    _lib.check_tensors(points.device, {"points": points, "table": table}, {"ray_grid_idx": ray_grid_idx})
    _lib.current_stream(points.device)  # (raises for anything but a GPU: there is no CPU path)
    grid_idx = _lib.int32_index(ray_grid_idx)
    cfg = _Cfg(layout, bool(mask_out_of_bounds_samples), bool(contract_coords))
    return _HashGridEncode.apply(cfg, points, table, grid_idx)

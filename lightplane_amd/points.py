"""The decoder at arbitrary 3-D points, fused into HIP (``csrc/lp_points.hip``; C ABI ``lp_points_forward`` / ``lp_points_backward``).

``lightplane_eval_mlp`` / ``lightplane_eval_mlp_opacity_only`` have the names and the argument order of the reference's functions
(naive_renderer.py:328-598), which its ``LightplaneRenderer.eval_decoder_at_points`` / ``eval_opacity_at_points`` call.  For point
``p = points[r, n]``, batch element ``ray_grid_idx[r]`` and encoding ``e = rays_encoding[r]``::

    q        = contract(p) if contract_coords else p
    features = sum over the grid-list of its tri- / bi-linear samples at q    (the Renderer's gather; 0 outside [-1, 1]^3 with the mask)
    t        = relu(trunk(features));  raw = opacity_mlp(t);  craw = color_mlp(t + e)
               (two-grid decoder: raw = opacity_mlp(relu(features)), craw = color_mlp(relu(color features) + e))
    opacity  = gain * softplus(raw) * occ;   colour = sigmoid(craw)[:color_chn] * occ;   occ = scaffold at q (1 without a scaffold)

One evaluation gives both results, and one ``torch.autograd.Function`` differentiates them jointly: gradients go to the grids, the
colour grids, ``mlp_params``, ``rays_encoding`` and ``points`` (the derivative of the interpolation weights, e.g. for surface normals;
the out-of-bounds mask and the scaffold are piecewise constant and contribute nothing).  Which gradients are computed follows
``requires_grad``; there is no double backward and no CPU path.  The backward reads nothing the forward wrote: it recomputes every
point's decoder.  Grids go to the kernels as they are -- a list of tensors that is never concatenated, or the flat ``[sum BDHW, C]``
tensor with ``grid_sizes``.  No host synchronisation (graph-capturable).

Deviations from the reference: the colour has ``color_chn`` channels, not the padded width of the colour head, and
``inject_opacity_noise`` other than ``None`` raises ``NotImplementedError``.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib
from .grids import GridForm, check_grid_and_color_grid
from .params import DecoderParams, int_list_of

__all__ = ["lightplane_eval_mlp", "lightplane_eval_mlp_opacity_only"]


class _Cfg(NamedTuple):
    grid: GridForm
    color_grid: Optional[GridForm]
    dims_t: tuple
    dims_o: tuple
    dims_c: tuple
    color_chn: int
    gain: float
    mask: bool
    contract: bool
    opacity_only: bool


def _fill(cfg: _Cfg, points, mlp_params, encoding, grid_idx, scaffold, grids, color_grids, with_color: bool) -> _lib.LpPointsArgs:
    a = _lib.LpPointsArgs()
    a.grid = cfg.grid.abi(grids)
    if with_color and cfg.color_grid is not None:
        a.color_grid = cfg.color_grid.abi(color_grids)
    a.mlp_params, a.n_mlp_params = _lib.ptr(mlp_params), mlp_params.numel()
    _lib.make_decoder(a, cfg.dims_t, cfg.dims_o, cfg.dims_c)
    a.color_chn, a.gain = cfg.color_chn, cfg.gain
    a.mask_out_of_bounds, a.contract_coords = int(cfg.mask), int(cfg.contract)
    a.points, a.grid_idx = _lib.ptr(points), _lib.ptr(grid_idx)
    if with_color:
        a.encoding, a.encoding_dim = _lib.ptr(encoding), encoding.shape[1]
    a.n_rays, a.n_pts = points.shape[0], points.shape[1]
    if scaffold is not None:
        a.scaffold = _lib.ptr(scaffold)
        a.scaffold_shape = _lib.LpGrid(*[int(v) for v in scaffold.shape], 0, None)
    return a


class _EvalPoints(torch.autograd.Function):
    """(opacity[, colour]) = decoder(points): one forward launch; the backward is one launch that recomputes the decoder and fills the
    gradients ``needs_input_grad`` asks for (a gradient nobody asks for is a NULL pointer: its work is skipped; an output nobody
    differentiated is a NULL upstream gradient: without one for the colour, the colour head is not evaluated)."""

    @staticmethod
    def forward(ctx, cfg: _Cfg, points, mlp_params, encoding, grid_idx, scaffold, *tensors):
        dev = points.device
        stream = _lib.current_stream(dev)
        points, mlp_params = _lib.aligned(points.contiguous()), _lib.aligned(mlp_params.contiguous())
        encoding = None if encoding is None else _lib.aligned(encoding.contiguous())
        n_g = cfg.grid.n_tensors
        grids, color_grids = tensors[:n_g], tensors[n_g:]
        n_rays, n_pts = points.shape[0], points.shape[1]
        with torch.cuda.device(dev):
            opacity = torch.empty(n_rays, n_pts, device=dev, dtype=torch.float32)
            color = None if cfg.opacity_only else torch.empty(n_rays, n_pts, cfg.color_chn, device=dev, dtype=torch.float32)
            a = _fill(cfg, points, mlp_params, encoding, grid_idx, scaffold, grids, color_grids, not cfg.opacity_only)
            a.opacity_out, a.color_out = _lib.ptr(opacity), _lib.ptr(color)
            _lib.check(_lib.lib().lp_points_forward(ctypes.byref(a), stream), "lp_points_forward")
        ctx.cfg = cfg
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(points, mlp_params, encoding, grid_idx, scaffold, *tensors)
        return opacity if cfg.opacity_only else (opacity, color)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_opacity, g_color=None):
        cfg: _Cfg = ctx.cfg
        points, mlp_params, encoding, grid_idx, scaffold, *tensors = ctx.saved_tensors
        need = ctx.needs_input_grad
        n_in = 6 + len(tensors)
        if (g_opacity is None and g_color is None) or not any(need):
            return (None,) * n_in
        dev = points.device
        stream = _lib.current_stream(dev)
        n_g = cfg.grid.n_tensors
        grids, color_grids = tensors[:n_g], tensors[n_g:]
        with_color = g_color is not None and not cfg.opacity_only
        g_opacity = None if g_opacity is None else _lib.aligned(g_opacity.to(torch.float32).contiguous())
        g_color = _lib.aligned(g_color.to(torch.float32).contiguous()) if with_color else None
        with torch.cuda.device(dev):
            d_points = torch.empty_like(points) if need[1] else None
            d_params = torch.zeros_like(mlp_params) if need[2] else None
            d_enc = torch.zeros_like(encoding) if (need[3] and encoding is not None) else None
            # (the library takes gradient buffers for every grid of a list or for none)
            d_grids = [torch.zeros_like(t) for t in grids] if any(need[6:6 + n_g]) else None
            d_cgrids = [torch.zeros_like(t) for t in color_grids] if (with_color and any(need[6 + n_g:])) else None
            a = _fill(cfg, points, mlp_params, encoding, grid_idx, scaffold, grids, color_grids, with_color)
            a.grad_opacity, a.grad_color = _lib.ptr(g_opacity), _lib.ptr(g_color)
            a.grad_points, a.grad_mlp_params = _lib.ptr(d_points), _lib.ptr(d_params)
            a.grad_encoding = _lib.ptr(d_enc) if with_color else None
            g_grids = _lib.route_grads(a, "grad_grid", cfg.grid, d_grids, need[6:6 + n_g])
            g_cgrids = _lib.route_grads(a, "grad_color_grid", cfg.color_grid, d_cgrids, need[6 + n_g:])
            _lib.check(_lib.lib().lp_points_backward(ctypes.byref(a), stream), "lp_points_backward")
        if d_cgrids is None:  # (the colour grids took no part: their gradient is zero, not absent)
            g_cgrids = tuple(torch.zeros_like(t) if n else None for t, n in zip(color_grids, need[6 + n_g:]))
        return (None, d_points, d_params, d_enc, None, None) + g_grids + g_cgrids


def _eval(points, grid, ray_grid_idx, decoder_params: DecoderParams, rays_encoding, gain, mask, noise, scaffold, color_grid, contract,
          grid_sizes, color_grid_sizes, opacity_only: bool):
    if noise is not None:
        raise NotImplementedError("inject_opacity_noise is not supported at points (pass None): the kernels add no noise here")
    assert torch.is_tensor(points) and points.ndim == 3 and points.shape[-1] == 3, "points has to be a [n_rays, n_pts, 3] tensor"
    n_rays = points.shape[0]
    assert torch.is_tensor(ray_grid_idx) and tuple(ray_grid_idx.shape) == (n_rays,), f"ray_grid_idx has to be a [{n_rays}] tensor"
    dims_t, dims_o, dims_c = (tuple(int_list_of(v)) for v in (decoder_params.n_hidden_trunk, decoder_params.n_hidden_opacity,
                                                              decoder_params.n_hidden_color))
    if opacity_only:
        color_grid, color_grid_sizes, rays_encoding = None, None, None
    else:
        assert torch.is_tensor(rays_encoding) and tuple(rays_encoding.shape) == (n_rays, dims_c[0]), (
            f"rays_encoding has to be a [{n_rays}, {dims_c[0]}] tensor (the colour head's input width)")
    check_grid_and_color_grid(grid, color_grid, grid_sizes, color_grid_sizes)
    grids, gform = GridForm.of(grid, grid_sizes, name="grid", sampler=False)
    cgrids, cform = ((), None) if color_grid is None else GridForm.of(color_grid, color_grid_sizes, name="color_grid", sampler=False)
    if cform is not None:
        assert len(dims_t) <= 1, "a decoder with a separate colour grid has no trunk layers"
    mlp_params = decoder_params.mlp_params
    assert mlp_params.ndim == 1, "decoder_params.mlp_params has to be the flat parameter vector"
    if scaffold is not None:
        assert torch.is_tensor(scaffold) and scaffold.ndim == 4, "scaffold has to be a [B, D, H, W] tensor"
    dev = points.device
    f32 = {"points": points, "decoder_params.mlp_params": mlp_params, "rays_encoding": rays_encoding, "scaffold": scaffold}
    _lib.check_grids(grids, "grid", f32, {"ray_grid_idx": ray_grid_idx}, device=dev)
    if cgrids:
        _lib.check_grids(cgrids, "color_grid", device=dev)
    grid_idx = _lib.int32_index(ray_grid_idx)
    scaffold = None if scaffold is None else _lib.aligned(scaffold.detach().contiguous())
    cfg = _Cfg(gform, cform, dims_t, dims_o, dims_c, int(decoder_params.color_chn), float(gain), bool(mask), bool(contract), opacity_only)
    return _EvalPoints.apply(cfg, points, mlp_params, rays_encoding, grid_idx, scaffold, *grids, *cgrids)


def lightplane_eval_mlp(points, grid, ray_grid_idx, decoder_params: DecoderParams, rays_encoding, gain: float,
                        mask_out_of_bounds_samples: bool = False, inject_opacity_noise=None, scaffold: Optional[torch.Tensor] = None,
                        color_grid=None, contract_coords: bool = False, *, grid_sizes=None,
                        color_grid_sizes=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(opacity [n_rays, n_pts], colour [n_rays, n_pts, color_chn])`` of the decoder at ``points [n_rays, n_pts, 3]`` (module
    docstring for the definition).

    ``grid`` / ``color_grid``: a *list* of ``[B, D, H, W, C]`` tensors, or a flat ``[sum BDHW, C]`` tensor with ``grid_sizes`` /
    ``color_grid_sizes``, as ``lightplane_renderer`` takes them; ``ray_grid_idx [n_rays]``: the batch element of each ray's points;
    ``rays_encoding [n_rays, E]``: added to the colour head's input; ``scaffold``: ``[B, D, H, W]`` occupancy or ``None``.
    Differentiable with respect to the grids, ``decoder_params.mlp_params``, ``rays_encoding`` and ``points``."""
    return _eval(points, grid, ray_grid_idx, decoder_params, rays_encoding, gain, mask_out_of_bounds_samples, inject_opacity_noise,
                 scaffold, color_grid, contract_coords, grid_sizes, color_grid_sizes, False)


def lightplane_eval_mlp_opacity_only(points, grid, ray_grid_idx, decoder_params: DecoderParams, gain: float,
                                     mask_out_of_bounds_samples: bool = False, inject_opacity_noise=None,
                                     scaffold: Optional[torch.Tensor] = None, contract_coords: bool = False, *,
                                     grid_sizes=None) -> torch.Tensor:
    """``opacity [n_rays, n_pts]`` alone: the opacity of ``lightplane_eval_mlp``, bit for bit, without the colour head -- there is no
    encoding and no colour grid, and the colour MLP's parameters are never read (they get exactly zero gradient)."""
    return _eval(points, grid, ray_grid_idx, decoder_params, None, gain, mask_out_of_bounds_samples, inject_opacity_noise,
                 scaffold, None, contract_coords, grid_sizes, None, True)

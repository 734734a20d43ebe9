"""Rendering at caller-given sample depths: the decoder and the compositing of the march in pieces in one launch
(``csrc/lp_render_samples.hip``; C ABI ``lp_render_samples_*`` of ``include/lightplane_hip_render_samples.h``).

    ray_samples | importance_samples  ->  render_samples

is the chain ``... -> lightplane_eval_mlp -> composite_samples`` without its per-sample tensors: sample ``s`` of ray ``r`` is evaluated
at ``depths[r, s] * direction + origin`` (formed in registers, contracted when asked; no points tensor exists), decoded as
``lightplane_eval_mlp`` decodes a point and composited as ``composite_samples`` does::

    w = T * (-expm1(-opacity * delta)),   ray_length = sum w depth,   -log T = sum opacity * delta,   feature = sum w colour

(opacity not clamped, no opacity noise, no early termination).  The fine pass of a coarse-to-fine march, and any importance-resampled
pass, runs through it; the fused Renderer places its samples uniformly only.

One ``torch.autograd.Function``: gradients go to the grids, the colour grids, ``decoder_params.mlp_params`` and ``rays.encoding``, from
all three results and from ``weights`` when they are returned (distortion and interlevel losses).  Autograd keeps the inputs and one
``[R, ceil(S / 64)]`` buffer -- the ``-log T`` every chunk of 64 samples starts from; the backward recomputes every sample's decoder.
``depths``, ``deltas``, ``rays.origins`` and ``rays.directions`` get NO gradient: if one of them requires one while grad mode is on
the call raises ``NotImplementedError`` (``.detach()`` them, or use the modular chain, which differentiates all four).
The forward and the encoding gradient are bit-reproducible; grid and parameter gradients are accumulated with atomics.  fp32, no host
synchronisation (graph-capturable), no double backward, no CPU path.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import torch

from . import _lib
from .grids import GridForm, check_grid_and_color_grid
from .params import DecoderParams, int_list_of
from .rays import Rays

__all__ = ["render_samples"]


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
    return_weights: bool


def chunks(n_samples: int) -> int:
    """Floats per ray of the buffer the forward leaves for the backward (``lp_render_samples_chunks``): ``ceil(n_samples / 64)``."""
    return (int(n_samples) + 63) // 64 if n_samples >= 1 else 0


def _fill(cfg: _Cfg, origins, directions, grid_idx, encoding, depths, deltas, mlp_params, scaffold, grids, color_grids):
    a = _lib.LpRenderSamplesArgs()
    a.grid = cfg.grid.abi(grids)
    if cfg.color_grid is not None:
        a.color_grid = cfg.color_grid.abi(color_grids)
    a.mlp_params, a.n_mlp_params = _lib.ptr(mlp_params), mlp_params.numel()
    _lib.make_decoder(a, cfg.dims_t, cfg.dims_o, cfg.dims_c)
    a.color_chn, a.gain = cfg.color_chn, cfg.gain
    a.mask_out_of_bounds, a.contract_coords = int(cfg.mask), int(cfg.contract)
    a.origins, a.directions, a.grid_idx = _lib.ptr(origins), _lib.ptr(directions), _lib.ptr(grid_idx)
    a.encoding, a.encoding_dim = _lib.ptr(encoding), encoding.shape[1]
    a.n_rays, a.n_samples = depths.shape
    a.depths, a.deltas = _lib.ptr(depths), _lib.ptr(deltas)
    if scaffold is not None:
        a.scaffold = _lib.ptr(scaffold)
        a.scaffold_shape = _lib.LpGrid(*[int(v) for v in scaffold.shape], 0, None)
    return a


class _RenderSamples(torch.autograd.Function):
    """(ray_length, -log T, feature[, weights]) = render(depths, deltas; grids, decoder, encoding): one forward launch; the backward is
    one launch that recomputes the decoder and fills the gradients ``needs_input_grad`` asks for (a gradient nobody asks for is a NULL
    pointer: its work is skipped; a result nobody differentiated is a NULL upstream gradient)."""

    @staticmethod
    def forward(ctx, cfg: _Cfg, origins, directions, grid_idx, depths, deltas, scaffold, mlp_params, encoding, *tensors):
        dev = depths.device
        stream = _lib.current_stream(dev)
        origins, directions, depths, deltas, mlp_params, encoding = (
            _lib.aligned(t.contiguous()) for t in (origins, directions, depths, deltas, mlp_params, encoding))
        n_g = cfg.grid.n_tensors
        grids, color_grids = tensors[:n_g], tensors[n_g:]
        n, s = depths.shape
        with torch.cuda.device(dev):
            length = torch.empty(n, device=dev, dtype=torch.float32)
            nlt = torch.empty(n, device=dev, dtype=torch.float32)
            feature = torch.empty(n, cfg.color_chn, device=dev, dtype=torch.float32)
            weights = torch.empty(n, s, device=dev, dtype=torch.float32) if cfg.return_weights else None
            chunk_nlt = torch.empty(n, chunks(s), device=dev, dtype=torch.float32)
            a = _fill(cfg, origins, directions, grid_idx, encoding, depths, deltas, mlp_params, scaffold, grids, color_grids)
            a.ray_length, a.neg_log_t, a.feature, a.weights = (_lib.ptr(t) for t in (length, nlt, feature, weights))
            a.chunk_nlt = _lib.ptr(chunk_nlt)
            _lib.check(_lib.lib().lp_render_samples_forward(ctypes.byref(a), stream), "lp_render_samples_forward")
        ctx.cfg = cfg
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(origins, directions, grid_idx, depths, deltas, scaffold, mlp_params, encoding, chunk_nlt, *tensors)
        return tuple(t for t in (length, nlt, feature, weights) if t is not None)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_len, g_nlt, g_feat, g_w=None):
        cfg: _Cfg = ctx.cfg
        origins, directions, grid_idx, depths, deltas, scaffold, mlp_params, encoding, chunk_nlt, *tensors = ctx.saved_tensors
        need = ctx.needs_input_grad
        n_in = 9 + len(tensors)
        ups = (g_len, g_nlt, g_feat, g_w)
        if all(g is None for g in ups) or not any(need):
            return (None,) * n_in
        dev = depths.device
        stream = _lib.current_stream(dev)
        n_g = cfg.grid.n_tensors
        grids, color_grids = tensors[:n_g], tensors[n_g:]
        g_len, g_nlt, g_feat, g_w = (None if g is None else _lib.aligned(g.to(torch.float32).contiguous()) for g in ups)
        with torch.cuda.device(dev):
            d_params = torch.zeros_like(mlp_params) if need[7] else None
            d_enc = torch.empty_like(encoding) if need[8] else None  # (written entirely: a ray is one wavefront's)
            # (the library takes gradient buffers for every grid of a list or for none)
            d_grids = [torch.zeros_like(t) for t in grids] if any(need[9:9 + n_g]) else None
            d_cgrids = [torch.zeros_like(t) for t in color_grids] if any(need[9 + n_g:]) else None
            a = _fill(cfg, origins, directions, grid_idx, encoding, depths, deltas, mlp_params, scaffold, grids, color_grids)
            a.chunk_nlt = _lib.ptr(chunk_nlt)
            a.grad_ray_length, a.grad_neg_log_t, a.grad_feature, a.grad_weights = (_lib.ptr(g) for g in (g_len, g_nlt, g_feat, g_w))
            a.grad_mlp_params, a.grad_encoding = _lib.ptr(d_params), _lib.ptr(d_enc)
            g_grids = _lib.route_grads(a, "grad_grid", cfg.grid, d_grids, need[9:9 + n_g])
            g_cgrids = _lib.route_grads(a, "grad_color_grid", cfg.color_grid, d_cgrids, need[9 + n_g:]) if color_grids else ()
            _lib.check(_lib.lib().lp_render_samples_backward(ctypes.byref(a), stream), "lp_render_samples_backward")
        return (None, None, None, None, None, None, None, d_params, d_enc) + g_grids + g_cgrids


def render_samples(rays: Rays, depths: torch.Tensor, deltas: torch.Tensor, grid, decoder_params: DecoderParams, *, gain: float = 1.0,
                   mask_out_of_bounds_samples: bool = False, contract_coords: bool = False, scaffold: Optional[torch.Tensor] = None,
                   color_grid=None, grid_sizes=None, color_grid_sizes=None, return_weights: bool = False):
    """``(ray_length_render [R], negative_log_transmittance [R], feature_render [R, color_chn])`` -- the Renderer's results -- of
    ``rays`` marched at the caller's ``depths [R, S]`` with the interval lengths ``deltas [R, S]`` (fp32; what ``composite_samples``
    takes: typically ``RaySamples.depths`` / ``.deltas`` of ``ray_samples`` or ``importance_samples``); with ``return_weights=True`` a
    fourth result, the compositing weights ``w [R, S]``.  Any ``S >= 1`` with ``R * S < 2^31``.

    Of ``rays`` the op reads ``origins``, ``directions``, ``grid_idx`` and ``encoding`` (``near`` and ``far`` are ignored).  ``grid`` /
    ``color_grid`` (a list of ``[B, D, H, W, C]`` tensors, or a flat ``[sum BDHW, C]`` tensor with ``grid_sizes`` /
    ``color_grid_sizes``), ``decoder_params``, ``gain``, ``mask_out_of_bounds_samples``, ``contract_coords`` and ``scaffold`` mean what
    they mean in ``lightplane_eval_mlp``.  Differentiable with respect to the grids, ``decoder_params.mlp_params`` and
    ``rays.encoding``; ``depths``, ``deltas``, ``rays.origins`` and ``rays.directions`` must not require a gradient (module docstring)."""
    assert isinstance(rays, Rays), f"rays has to be a Rays object, got {type(rays).__name__}"
    assert torch.is_tensor(depths) and depths.ndim == 2, "depths has to be a [n_rays, n_samples] tensor"
    n, s = depths.shape
    assert s >= 1, "depths has to have one sample per ray at least"
    assert torch.is_tensor(deltas) and tuple(deltas.shape) == (n, s), f"deltas has to be a [{n}, {s}] tensor, as depths is"
    assert n * s < 2 ** 31, f"depths: {n} rays x {s} samples: n_rays * n_samples has to stay below 2^31 (split the batch)"
    for name, t in (("rays.origins", rays.origins), ("rays.directions", rays.directions)):
        assert torch.is_tensor(t) and tuple(t.shape) == (n, 3), f"{name} has to be a [{n}, 3] tensor: one ray per row of depths"
    assert torch.is_tensor(rays.grid_idx) and tuple(rays.grid_idx.shape) == (n,), f"rays.grid_idx has to be a [{n}] tensor"
    dims_t, dims_o, dims_c = (tuple(int_list_of(v)) for v in (decoder_params.n_hidden_trunk, decoder_params.n_hidden_opacity,
                                                              decoder_params.n_hidden_color))
    encoding = rays.encoding
    assert torch.is_tensor(encoding) and tuple(encoding.shape) == (n, dims_c[0]), (
        f"rays.encoding has to be a [{n}, {dims_c[0]}] tensor (the colour head's input width)")
    if torch.is_grad_enabled():
        for name, t in (("depths", depths), ("deltas", deltas), ("rays.origins", rays.origins), ("rays.directions", rays.directions)):
            if t.requires_grad:
                raise NotImplementedError(
                    f"{name} requires a gradient, and render_samples produces none for depths, deltas, ray origins and directions: pass "
                    f"{name}.detach(), or use the modular chain (ray_samples / importance_samples -> lightplane_eval_mlp -> "
                    "composite_samples), which differentiates with respect to them")
    check_grid_and_color_grid(grid, color_grid, grid_sizes, color_grid_sizes)
    grids, gform = GridForm.of(grid, grid_sizes, name="grid", sampler=False)
    cgrids, cform = ((), None) if color_grid is None else GridForm.of(color_grid, color_grid_sizes, name="color_grid", sampler=False)
    if cform is not None:
        assert len(dims_t) <= 1, "a decoder with a separate colour grid has no trunk layers"
    mlp_params = decoder_params.mlp_params
    assert mlp_params.ndim == 1, "decoder_params.mlp_params has to be the flat parameter vector"
    if scaffold is not None:
        assert torch.is_tensor(scaffold) and scaffold.ndim == 4, "scaffold has to be a [B, D, H, W] tensor"
    f32 = {"depths": depths, "deltas": deltas, "rays.origins": rays.origins, "rays.directions": rays.directions,
           "decoder_params.mlp_params": mlp_params, "rays.encoding": encoding, "scaffold": scaffold}
    dev = _lib.check_grids(grids, "grid", f32, {"rays.grid_idx": rays.grid_idx})  # (every tensor on the grid's GPU)
    if cgrids:
        _lib.check_grids(cgrids, "color_grid", device=dev)
    grid_idx = _lib.int32_index(rays.grid_idx)
    scaffold = None if scaffold is None else _lib.aligned(scaffold.detach().contiguous())
    cfg = _Cfg(gform, cform, dims_t, dims_o, dims_c, int(decoder_params.color_chn), float(gain), bool(mask_out_of_bounds_samples),
               bool(contract_coords), bool(return_weights))
    return _RenderSamples.apply(cfg, rays.origins.detach(), rays.directions.detach(), grid_idx, depths.detach(), deltas.detach(), scaffold,
                                mlp_params, encoding, *grids, *cgrids)

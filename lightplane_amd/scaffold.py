"""Occupancy scaffold of a grid-list, fused into HIP (``csrc/lp_scaffold.hip``; C ABI ``lp_scaffold_*``).

The decoder's opacity ``gain * softplus(opacity_mlp(relu(trunk_mlp(sample(grid, p)))))`` -- with a decoder without trunk layers (the
two-grid mode), ``opacity_mlp(relu(sample(grid, p)))`` -- on the regular lattice of a ``[B, D, H, W]`` scaffold::

    p[z, y, x] = (lin(W)[x], lin(H)[y], lin(D)[z]),   lin(n) = torch.linspace(0, 1, n) * 2 - 1

thresholded and dilated: ``max_pool3d(opacity, 2 r + 1, stride=1, padding=r) > threshold`` as 0 / 1 floats -- the reference's
``LightplaneRenderer.calculate_scaffold`` (renderer_module.py:349-417).  The kernel forms the lattice coordinates itself, so no point,
ray or encoding tensor exists; the colour MLP is never evaluated; and because the pool's ``-inf`` padding never wins and ``max``
commutes with the monotone map ``v -> v > threshold``, the pool is computed as a separable OR-dilation of occupancy *bytes*.  Memory
beyond the ``4 B D H W`` bytes of the result: ``scaffold_workspace_bytes`` (one byte per lattice point, nothing without dilation).
The grid goes to the kernels as it is -- a list of tensors that is never concatenated, or the flat ``[sum BDHW, C]`` tensor with
``grid_sizes``.  No gradient (a scaffold has none), no host synchronisation (graph-capturable), no atomics (bit-reproducible).
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib
from .grids import GridForm
from .params import DecoderParams, int_list_of

__all__ = ["calculate_scaffold", "scaffold_opacity", "scaffold_workspace_bytes"]


def _shape(scaffold_size):
    if torch.is_tensor(scaffold_size):
        scaffold_size = scaffold_size.tolist()
    size = [int(v) for v in scaffold_size]
    assert len(size) == 4 and all(v >= 1 for v in size), f"scaffold_size has to be a positive [B, D, H, W], got {size}"
    return size


def scaffold_workspace_bytes(scaffold_size, dilate_scaffold: int) -> int:
    """Bytes of device workspace ``calculate_scaffold`` takes for a scaffold of ``[B, D, H, W]`` points (``lp_scaffold_workspace_bytes``;
    shapes only, no GPU): one byte per point when ``dilate_scaffold > 0``, else 0."""
    a = _lib.LpScaffoldArgs()
    a.shape = _lib.LpGrid(*_shape(scaffold_size), 0, None)
    a.dilate = int(dilate_scaffold)
    return _lib.query(_lib.lib().lp_scaffold_workspace_bytes, ctypes.byref(a), what="lp_scaffold_workspace_bytes")


def _args(feature_grid, decoder_params: DecoderParams, scaffold_size, gain, threshold, dilate, mask, grid_sizes):
    """``(args, device, keep-alive tensors)``: the argument block of one call.  The grid tensors go in as they are (contiguous, on one
    GPU, fp32 -- checked, never copied); the library refuses a base that is not 16-byte aligned."""
    tensors, form = GridForm.of(feature_grid, grid_sizes, name="feature_grid", sampler=False)
    size = _shape(scaffold_size)
    dims_t, dims_o = int_list_of(decoder_params.n_hidden_trunk), int_list_of(decoder_params.n_hidden_opacity)
    mlp_params = decoder_params.mlp_params
    assert torch.is_tensor(mlp_params), "decoder_params.mlp_params has to be a tensor"
    assert mlp_params.ndim == 1, "decoder_params.mlp_params has to be the flat parameter vector"
    dev = _lib.check_grids(tensors, "feature_grid", {"decoder_params.mlp_params": mlp_params})
    mlp_params = _lib.aligned(mlp_params.detach().contiguous())
    a = _lib.LpScaffoldArgs()
    a.grid = form.abi(tensors)
    a.mlp_params, a.n_mlp_params = _lib.ptr(mlp_params), mlp_params.numel()
    _lib.make_decoder(a, dims_t, dims_o)
    a.gain, a.mask_out_of_bounds = float(gain), int(bool(mask))
    a.shape = _lib.LpGrid(*size, 0, None)
    a.threshold, a.dilate = float(threshold), int(dilate)
    return a, dev, size, (tensors, mlp_params)


@torch.no_grad()
def scaffold_opacity(feature_grid, decoder_params: DecoderParams, scaffold_size, *, gain: float = 1.0,
                     mask_out_of_bounds_samples: bool = False, grid_sizes=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The decoder's opacity on the lattice of a ``[B, D, H, W]`` scaffold, ``[B, D, H, W]`` fp32 (module docstring): what
    ``calculate_scaffold`` thresholds, for parity checks and diagnostics.  ``out``: a contiguous fp32 result tensor to write into."""
    a, dev, size, keep = _args(feature_grid, decoder_params, scaffold_size, gain, 0.0, 0, mask_out_of_bounds_samples, grid_sizes)
    with torch.cuda.device(dev):
        out = _result(out, size, dev)
        _lib.check(_lib.lib().lp_scaffold_opacity(ctypes.byref(a), out.data_ptr(), _lib.current_stream(dev)), "lp_scaffold_opacity")
    del keep
    return out


@torch.no_grad()
def calculate_scaffold(feature_grid, decoder_params: DecoderParams, scaffold_size, *, gain: float = 1.0, threshold: float = 1e-7,
                       dilate_scaffold: int = 2, mask_out_of_bounds_samples: bool = False, grid_sizes=None,
                       out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Occupancy scaffold ``[B, D, H, W]`` (0 / 1 floats) of a grid-list under a decoder (module docstring for the definition).

    ``feature_grid``: a *list* of ``[B, D, H, W, C]`` tensors or a flat ``[sum BDHW, C]`` tensor with ``grid_sizes``, as
    ``lightplane_renderer`` takes them; ``decoder_params``: the Renderer's (the colour MLP is not read).  ``dilate_scaffold``: radius
    ``r`` of the ``2 r + 1`` window, 0 = none.  ``out`` / ``workspace``: optional preallocated result (contiguous fp32
    ``[B, D, H, W]``) and uint8 workspace of at least ``scaffold_workspace_bytes`` elements, e.g. for graph capture; allocated otherwise."""
    assert int(dilate_scaffold) >= 0, f"dilate_scaffold has to be >= 0, got {dilate_scaffold!r}"
    a, dev, size, keep = _args(feature_grid, decoder_params, scaffold_size, gain, threshold, dilate_scaffold,
                               mask_out_of_bounds_samples, grid_sizes)
    L = _lib.lib()
    need = _lib.query(L.lp_scaffold_workspace_bytes, ctypes.byref(a), what="lp_scaffold_workspace_bytes")
    with torch.cuda.device(dev):
        out = _result(out, size, dev)
        if need > 0:
            if workspace is None:
                workspace = torch.empty(need, dtype=torch.uint8, device=dev)
            assert (workspace.dtype == torch.uint8 and workspace.device == dev and workspace.is_contiguous()
                    and workspace.numel() >= need), f"workspace has to be a contiguous uint8 tensor of >= {need} elements on {dev}"
        ws_ptr, ws_bytes = (workspace.data_ptr(), workspace.numel()) if need > 0 else (None, 0)
        _lib.check(L.lp_scaffold_build(ctypes.byref(a), out.data_ptr(), ws_ptr, ws_bytes, _lib.current_stream(dev)), "lp_scaffold_build")
    del keep
    return out


def _result(out, size, dev) -> torch.Tensor:
    if out is None:
        return torch.empty(size, dtype=torch.float32, device=dev)
    assert (out.dtype == torch.float32 and out.device == dev and out.is_contiguous() and list(out.shape) == list(size)), (
        f"out has to be a contiguous float32 tensor of shape {size} on {dev}")
    return out

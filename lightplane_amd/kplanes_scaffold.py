"""Occupancy scaffold of a space-time plane field (``kplanes.py``) over a set of timestamps, fused into HIP
(``csrc/lp_kplanes_scaffold.hip``; C ABI ``lp_kplanes_scaffold_*``): the ``[B, D, H, W]`` lattice that ``kplanes_eval_mlp``,
``kplanes_render_samples``, ``clip_rays_to_scaffold`` and ``marching_cubes`` consume, produced from the planes themselves::

    p[z, y, x]          = (lin(W)[x], lin(H)[y], lin(D)[z]),   lin(n) = torch.linspace(0, 1, n) * 2 - 1
    opacity[b, z, y, x] = max over t in times of  gain * softplus(opacity_mlp(relu(trunk_mlp(feat(p[z, y, x], t)))))
    scaffold            = max_pool3d(opacity, 2 r + 1, stride=1, padding=r) > threshold        (0 / 1 floats)

``feat`` is exactly the encoding of ``kplanes_encode`` for batch element ``b``; a decoder without trunk layers reads ``relu(feat)``, as
everywhere else.  There is no ``mask_out_of_bounds_samples`` and no ``contract_coords``: every lattice point lies inside the cube, and
a scaffold is looked up at the already contracted coordinate.  ``times`` is a 1-D fp32 tensor ``[T]``, ``T >= 1``, read on the device:
any values in any order, a time outside ``[-1, 1]`` clamps as in the encoding; a static layout takes ``None``.  ``T = 1`` is the
opacity lattice at one instant: ``marching_cubes(kplanes_scaffold_opacity(..., times=t[None]), level)`` is the mesh of the field then.

One lattice launch: no lattice points, no features and no per-timestamp opacity reach memory, the lookups that do not depend on ``x``
are made once per lattice row and the loop over the timestamps runs inside the kernel.  Memory beyond the ``4 B D H W`` bytes of the
result: ``kplanes_scaffold_workspace_bytes`` (one byte per lattice point, nothing without dilation).  No gradient, no host
synchronisation (graph-capturable), no atomics (bit-reproducible); the colour MLP is never read.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib
from .kplanes import KPlanesLayout
from .params import DecoderParams, int_list_of
from .scaffold import _result, _shape

__all__ = ["kplanes_calculate_scaffold", "kplanes_scaffold_opacity", "kplanes_scaffold_workspace_bytes"]


def kplanes_scaffold_workspace_bytes(scaffold_size, dilate_scaffold: int) -> int:
    """Bytes of device workspace ``kplanes_calculate_scaffold`` takes for a scaffold of ``[B, D, H, W]`` points
    (``lp_kplanes_scaffold_workspace_bytes``; shapes only, no GPU): one byte per point when ``dilate_scaffold > 0``, else 0."""
    a = _lib.LpKPlanesScaffoldArgs()
    a.shape = _lib.LpGrid(*_shape(scaffold_size), 0, None)
    a.dilate = int(dilate_scaffold)
    return _lib.query(_lib.lib().lp_kplanes_scaffold_workspace_bytes, ctypes.byref(a), what="lp_kplanes_scaffold_workspace_bytes")


def _args(planes, layout: KPlanesLayout, decoder_params: DecoderParams, scaffold_size, times, gain, threshold, dilate):
    """``(args, device, size, keep-alive tensors)``: the checks that need no device, then the argument block of one call."""
    if not isinstance(layout, KPlanesLayout):
        raise ValueError("layout has to be the KPlanesLayout of kplanes_layout()")
    if not torch.is_tensor(planes) or planes.ndim != 3 or planes.shape[0] < 1 or tuple(planes.shape[1:]) != (layout.rows, layout.channels):
        shape = tuple(planes.shape) if torch.is_tensor(planes) else type(planes).__name__
        raise ValueError(f"planes has to be a [B, {layout.rows}, {layout.channels}] tensor for this layout (got {shape})")
    if layout.n_planes == 3:
        if times is not None:
            raise ValueError("times has to be None for a static layout (time_resolution=None)")
    elif not torch.is_tensor(times) or times.ndim != 1 or times.numel() < 1:
        raise ValueError("times has to be a 1-D tensor [T], T >= 1, for a dynamic layout")
    size = _shape(scaffold_size)
    if size[0] != planes.shape[0]:
        raise ValueError(f"scaffold_size[0] = {size[0]} has to be the batch size {planes.shape[0]} of planes")
    assert size[0] * size[1] * size[2] * size[3] < 1 << 31, f"scaffold_size {size}: the lattice has to stay below 2^31 points"
    dims_t, dims_o = tuple(int_list_of(decoder_params.n_hidden_trunk)), tuple(int_list_of(decoder_params.n_hidden_opacity))
    width = dims_t[0] if len(dims_t) > 1 else dims_o[0]
    if width != layout.out_channels:
        raise ValueError(f"the decoder reads {width} features, the layout has n_scales x channels = {layout.out_channels}")
    mlp_params = decoder_params.mlp_params
    assert torch.is_tensor(mlp_params) and mlp_params.ndim == 1, "decoder_params.mlp_params has to be the flat parameter vector"
    dev = planes.device
    _lib.check_tensors(dev, {"planes": planes, "times": times, "decoder_params.mlp_params": mlp_params})
    _lib.current_stream(dev)  # (raises for anything but a GPU: there is no CPU path)
    planes = _lib.aligned(planes.detach().contiguous(), grid=True)
    mlp_params = _lib.aligned(mlp_params.detach().contiguous())
    times = None if times is None else _lib.aligned(times.detach().contiguous())
    a = _lib.LpKPlanesScaffoldArgs()
    a.planes, a.times, a.n_times = _lib.ptr(planes), _lib.ptr(times), 0 if times is None else times.numel()
    a.batch, a.rows = planes.shape[0], layout.rows
    a.channels, a.n_scales, a.n_planes = layout.channels, layout.n_scales, layout.n_planes
    for s in range(layout.n_scales):
        a.spatial[s] = layout.spatial[s]
        a.temporal[s] = layout.temporal[s] if layout.temporal else 0
        for j in range(layout.n_planes):
            a.offset[s][j] = layout.offsets[s][j]
    a.mlp_params, a.n_mlp_params = _lib.ptr(mlp_params), mlp_params.numel()
    _lib.make_decoder(a, dims_t, dims_o)
    a.gain, a.threshold, a.dilate = float(gain), float(threshold), int(dilate)
    a.shape = _lib.LpGrid(*size, 0, None)
    return a, dev, size, (planes, times, mlp_params)


@torch.no_grad()
def kplanes_scaffold_opacity(planes, layout: KPlanesLayout, decoder_params: DecoderParams, scaffold_size, *, times=None,
                             gain: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The decoder's opacity on the lattice of a ``[B, D, H, W]`` scaffold, maximised over ``times``: ``[B, D, H, W]`` fp32 (module
    docstring) -- what ``kplanes_calculate_scaffold`` thresholds, and with one timestamp the volume ``marching_cubes`` takes.
    ``planes [B, layout.rows, C]``, ``layout``: as ``kplanes_encode``; ``scaffold_size[0]`` has to be ``B``; ``out``: a contiguous
    fp32 result tensor to write into.  There is neither a mask nor a contraction (module docstring)."""
    a, dev, size, keep = _args(planes, layout, decoder_params, scaffold_size, times, gain, 0.0, 0)
    with torch.cuda.device(dev):
        out = _result(out, size, dev)
        _lib.check(_lib.lib().lp_kplanes_scaffold_opacity(ctypes.byref(a), out.data_ptr(), _lib.current_stream(dev)),
                   "lp_kplanes_scaffold_opacity")
    del keep
    return out


@torch.no_grad()
def kplanes_calculate_scaffold(planes, layout: KPlanesLayout, decoder_params: DecoderParams, scaffold_size, *, times=None,
                               gain: float = 1.0, threshold: float = 1e-7, dilate_scaffold: int = 2,
                               out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Occupancy scaffold ``[B, D, H, W]`` (0 / 1 floats) of a plane field under a decoder over the timestamps ``times`` (module
    docstring for the definition): a point is occupied when it, or a point within ``dilate_scaffold`` lattice steps of it, is more
    opaque than ``threshold`` at any of the timestamps.  There is neither a mask nor a contraction: every lattice point lies inside
    the cube, and a scaffold is looked up at the already contracted coordinate.  ``out`` / ``workspace``: optional preallocated result
    (contiguous fp32 ``[B, D, H, W]``) and uint8 workspace of at least ``kplanes_scaffold_workspace_bytes`` elements, e.g. for graph
    capture; allocated otherwise."""
    assert int(dilate_scaffold) >= 0, f"dilate_scaffold has to be >= 0, got {dilate_scaffold!r}"
    a, dev, size, keep = _args(planes, layout, decoder_params, scaffold_size, times, gain, threshold, dilate_scaffold)
    L = _lib.lib()
    need = _lib.query(L.lp_kplanes_scaffold_workspace_bytes, ctypes.byref(a), what="lp_kplanes_scaffold_workspace_bytes")
    with torch.cuda.device(dev):
        out = _result(out, size, dev)
        if need > 0:
            if workspace is None:
                workspace = torch.empty(need, dtype=torch.uint8, device=dev)
            assert (workspace.dtype == torch.uint8 and workspace.device == dev and workspace.is_contiguous()
                    and workspace.numel() >= need), f"workspace has to be a contiguous uint8 tensor of >= {need} elements on {dev}"
        ws_ptr, ws_bytes = (workspace.data_ptr(), workspace.numel()) if need > 0 else (None, 0)
        _lib.check(L.lp_kplanes_scaffold_build(ctypes.byref(a), out.data_ptr(), ws_ptr, ws_bytes, _lib.current_stream(dev)),
                   "lp_kplanes_scaffold_build")
    del keep
    return out

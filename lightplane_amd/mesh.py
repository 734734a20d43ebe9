"""Triangle mesh of a grid-list, fused into HIP (``csrc/lp_mesh.hip``; C ABI ``lp_mesh_*``): marching cubes on the GPU.

``marching_cubes`` meshes the level set ``{volume = level}`` of a ``[B, D, H, W]`` lattice whose point ``[z, y, x]`` sits at the
scaffold's coordinates::

    p[z, y, x] = (lin(W)[x], lin(H)[y], lin(D)[z]),   lin(n) = torch.linspace(-1, 1, n)

A point is inside when ``volume >= level`` (a NaN is outside); a lattice edge with exactly one endpoint inside carries the vertex
``p_lo + t (p_hi - p_lo)``, ``t = clamp((level - v_lo) / (v_hi - v_lo), 0, 1)``; every cell contributes the triangles of a generated
table (``scripts/gen_mc_table.py``) that is watertight by construction, with normals towards the lower values.  Two streaming passes
over the lattice and a scan between them, no atomics.  The output order is part of the contract: vertices by owner point (the edge's
endpoint with the lower coordinate, in the lattice's memory order) and axis x, y, z; faces by cell and table order; the scenes of a
batch concatenated, with ``vertex_offsets`` / ``face_offsets`` (``[B + 1]`` int64) and vertex ids local to their scene.  The result is
bit-reproducible.  A surface that reaches the lattice border is open there; an axis of size 1 has no cells and gives an empty mesh.

``extract_mesh`` is ``scaffold_opacity`` followed by ``marching_cubes`` and, with a ray encoding, ``lightplane_eval_mlp`` at the
vertices.  No gradient, no CPU path.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import torch

from . import _lib
from .params import DecoderParams
from .points import lightplane_eval_mlp
from .scaffold import scaffold_opacity

__all__ = ["marching_cubes", "extract_mesh", "mesh_workspace_bytes", "Mesh", "ColoredMesh"]


class Mesh(NamedTuple):
    vertices: torch.Tensor          # [V, 3] fp32, scene coordinates (x, y, z)
    faces: torch.Tensor             # [F, 3] int32, vertex ids local to the face's scene
    normals: Optional[torch.Tensor]  # [V, 3] fp32 unit vectors along -grad, or None
    vertex_offsets: torch.Tensor    # [B + 1] int64 on the GPU: scene b owns vertices[vertex_offsets[b]:vertex_offsets[b + 1]]
    face_offsets: torch.Tensor      # [B + 1] int64 on the GPU


class ColoredMesh(NamedTuple):
    vertices: torch.Tensor
    faces: torch.Tensor
    normals: Optional[torch.Tensor]
    vertex_offsets: torch.Tensor
    face_offsets: torch.Tensor
    colors: Optional[torch.Tensor]  # [V, color_chn] fp32, or None without a ray encoding


def _shape(volume_size):
    if torch.is_tensor(volume_size):
        volume_size = volume_size.tolist()
    size = [int(v) for v in volume_size]
    if len(size) == 3:
        size = [1] + size
    assert len(size) == 4 and all(v >= 1 for v in size), f"volume_size has to be a positive [B, D, H, W] or [D, H, W], got {size}"
    return size


def mesh_workspace_bytes(volume_size) -> int:
    """Bytes of device workspace ``marching_cubes`` takes for a ``[B, D, H, W]`` (or ``[D, H, W]``) lattice (``lp_mesh_workspace_bytes``;
    shapes only, no GPU): 4 bytes per lattice point, 16 bytes per 256 points and the small upper levels of the scan."""
    a = _lib.LpMeshArgs()
    a.shape = _lib.LpGrid(*_shape(volume_size), 0, None)
    return _lib.query(_lib.lib().lp_mesh_workspace_bytes, ctypes.byref(a), what="lp_mesh_workspace_bytes")


@torch.no_grad()
def marching_cubes(volume: torch.Tensor, level: float, *, with_normals: bool = False, max_vertices: Optional[int] = None,
                   max_faces: Optional[int] = None, workspace: Optional[torch.Tensor] = None) -> Mesh:
    """Mesh of ``{volume = level}`` (module docstring for the definition and the ordering contract).

    ``volume``: a contiguous fp32 ``[B, D, H, W]`` or ``[D, H, W]`` tensor on the GPU, 16-byte aligned (it is never copied: anything
    else is refused).  ``with_normals``: also the unit vectors along ``-grad volume`` at the vertices (central differences in scene
    coordinates, one-sided at the border, interpolated along the edge; ``(0, 0, 0)`` where the gradient vanishes).

    Default mode: the results have exactly the mesh's size.  That takes ONE host synchronisation -- the two offset arrays (their last
    entries are the totals) are read from the device between the count and the emit pass.

    Capacity mode (``max_vertices`` and ``max_faces`` both given): no host synchronisation, graph-capturable.  The results have the
    capacities' sizes; elements at or beyond the true counts are not written, and nothing is written beyond a capacity.  The true
    counts come back on the device, as ``vertex_offsets[-1]`` and ``face_offsets[-1]``: a count above its capacity means the mesh
    did not fit (what was written is the part below the capacity).

    ``workspace``: optional uint8 tensor of at least ``mesh_workspace_bytes(volume.shape)`` elements; allocated otherwise."""
    return _marching_cubes(volume, level, with_normals, max_vertices, max_faces, workspace)[0]


def _marching_cubes(volume, level, with_normals, max_vertices, max_faces, workspace):
    """``(Mesh, host copy of vertex_offsets)``: ``marching_cubes`` and what its one host read of the default mode brought along (``None``
    in capacity mode, which reads nothing)."""
    assert torch.is_tensor(volume) and volume.ndim in (3, 4), "volume has to be a [B, D, H, W] or [D, H, W] tensor"
    assert (max_vertices is None) == (max_faces is None), "max_vertices and max_faces go together (capacity mode takes both)"
    dev = volume.device
    _lib.check_tensors(dev, {"volume": volume})
    assert volume.is_contiguous(), "volume handed to the HIP library must be contiguous"
    stream = _lib.current_stream(dev)  # (raises for anything but a GPU: there is no CPU path)
    size = _shape(volume.shape)
    volume = volume.detach()
    L = _lib.lib()
    a = _lib.LpMeshArgs()
    a.volume = volume.data_ptr()
    a.shape = _lib.LpGrid(*size, 0, None)
    a.level = float(level)
    need = _lib.query(L.lp_mesh_workspace_bytes, ctypes.byref(a), what="lp_mesh_workspace_bytes")
    with torch.cuda.device(dev):
        if workspace is None:
            workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        assert (workspace.dtype == torch.uint8 and workspace.device == dev and workspace.is_contiguous()
                and workspace.numel() >= need), f"workspace has to be a contiguous uint8 tensor of >= {need} elements on {dev}"
        vertex_offsets = torch.empty(size[0] + 1, dtype=torch.int64, device=dev)
        face_offsets = torch.empty(size[0] + 1, dtype=torch.int64, device=dev)
        a.vertex_offsets, a.face_offsets = vertex_offsets.data_ptr(), face_offsets.data_ptr()
        _lib.check(L.lp_mesh_count(ctypes.byref(a), workspace.data_ptr(), workspace.numel(), stream), "lp_mesh_count")
        host_offsets = None
        if max_vertices is None:
            # the one host synchronisation of the default mode: both offset arrays in one copy
            host_offsets, host_face_offsets = torch.stack((vertex_offsets, face_offsets)).tolist()
            n_v, n_f = int(host_offsets[-1]), int(host_face_offsets[-1])
        else:
            n_v, n_f = int(max_vertices), int(max_faces)
            assert n_v >= 0 and n_f >= 0, "max_vertices and max_faces have to be >= 0"
        vertices = torch.empty(n_v, 3, dtype=torch.float32, device=dev)
        faces = torch.empty(n_f, 3, dtype=torch.int32, device=dev)
        normals = torch.empty(n_v, 3, dtype=torch.float32, device=dev) if with_normals else None
        mesh = _emit(a, vertices, faces, normals, workspace, stream)
    return Mesh(mesh[0], mesh[1], mesh[2], vertex_offsets, face_offsets), host_offsets


def _emit(a, vertices, faces, normals, workspace, stream):
    """The emit pass of a counted lattice into caller tensors (``[n, 3]`` each; ``normals`` may be ``None``)."""
    a.max_vertices, a.max_faces = vertices.shape[0], faces.shape[0]
    a.vertices = vertices.data_ptr() if vertices.numel() else None
    a.faces = faces.data_ptr() if faces.numel() else None
    a.normals = normals.data_ptr() if (normals is not None and normals.numel()) else None
    _lib.check(_lib.lib().lp_mesh_emit(ctypes.byref(a), workspace.data_ptr(), workspace.numel(), stream), "lp_mesh_emit")
    return vertices, faces, normals


@torch.no_grad()
def extract_mesh(feature_grid, decoder_params: DecoderParams, lattice_size, *, level: float, gain: float = 1.0,
                 mask_out_of_bounds_samples: bool = False, grid_sizes=None, with_normals: bool = True,
                 rays_encoding: Optional[torch.Tensor] = None, color_grid=None, color_grid_sizes=None) -> ColoredMesh:
    """Mesh of the level set ``{opacity = level}`` of a grid-list under a decoder: ``scaffold_opacity`` on a ``[B, D, H, W]`` lattice
    followed by ``marching_cubes`` in its default mode.  One host synchronisation in all: the colouring below splits the vertices by
    scene with the offsets that read already brought to the host.

    ``feature_grid`` / ``color_grid``: a *list* of ``[B, D, H, W, C]`` tensors or flat ``[sum BDHW, C]`` tensors with ``grid_sizes`` /
    ``color_grid_sizes``, as ``lightplane_renderer`` takes them -- never copied.  ``rays_encoding [B, E]``: when given, the result
    also carries per-vertex colours, ``lightplane_eval_mlp`` at the vertices, one launch per non-empty scene -- one "ray" per scene with that scene's encoding, its
    vertices as the ray's points (``gain``, the mask and the colour grid as given; no scaffold, no contraction).  ``with_normals``:
    the normals ``-grad opacity / |grad opacity|`` of the lattice."""
    opacity = scaffold_opacity(feature_grid, decoder_params, lattice_size, gain=gain,
                               mask_out_of_bounds_samples=mask_out_of_bounds_samples, grid_sizes=grid_sizes)
    mesh, bounds = _marching_cubes(opacity, level, with_normals, None, None, None)
    del opacity
    colors = None
    if rays_encoding is not None:
        B = mesh.vertex_offsets.numel() - 1
        assert torch.is_tensor(rays_encoding) and rays_encoding.ndim == 2 and rays_encoding.shape[0] == B, (
            f"rays_encoding has to be a [{B}, E] tensor: one encoding per scene")
        dev = mesh.vertices.device
        colors = torch.empty(mesh.vertices.shape[0], int(decoder_params.color_chn), dtype=torch.float32, device=dev)
        for b in range(B):
            lo, hi = bounds[b], bounds[b + 1]
            if hi == lo:
                continue
            _, c = lightplane_eval_mlp(mesh.vertices[lo:hi][None], feature_grid, torch.full((1,), b, dtype=torch.int32, device=dev),
                                       decoder_params, rays_encoding[b:b + 1], gain, mask_out_of_bounds_samples, None, None, color_grid,
                                       False, grid_sizes=grid_sizes, color_grid_sizes=color_grid_sizes)
            colors[lo:hi] = c[0]
    return ColoredMesh(mesh.vertices, mesh.faces, mesh.normals, mesh.vertex_offsets, mesh.face_offsets, colors)

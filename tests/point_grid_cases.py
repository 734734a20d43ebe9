"""Inputs and fp64 oracle of the gather / splat at points (tests/test_point_grid_host.py checks the inputs without a GPU,
tests/test_gpu_point_grid.py holds the kernels to the oracle).  Every case is built once per process and never modified.

Oracle, in fp64 on the fp32 inputs: ``oracle.lightplane_oracle.sample_grid_list`` for the gather; its autograd adjoint for the raw
splat; ``F / clamp(W, 1e-5)`` with ``W`` the raw splat of ones for the normalised splat; autograd for every gradient.  All of them are
partial derivatives of ``B(G, P, U) = sum(sample_grid_list(G, q(P)) * U)``.

The interpolation weights are continuous across cell faces, so values need no exclusions there.  Treated specially:
* LEFT OUT of value comparisons, with the mask only: points within 1e-5 of a face of [-1, 1]^3 after the contraction (fp32 geometry
  may put them on the other side).  Their vectors are zeroed where they would reach a grid (splat values).  At most 2 % of a case; the
  weights of the normalised splat count every point, so the cases with the mask are seeded to have none at all.
* per-point vector ZEROED for the POINT gradient only (everything is linear in it per point, so such a point has no point gradient
  in the kernel and in the oracle alike): within 1e-3 of a cell of a cell face of any grid (the weights have a kink), within 1e-3 of
  the kink of the contraction (tests/points_cases.py's rule), and the points left out above.  At most 5 % of a case.
A seed that misses a cap is changed, never the bar.
"""
import torch

from oracle import lightplane_oracle as O
from tests.synth import grid_sizes_for

TOL = 1e-4          # the project's bar: max |err| / max |ref|
CELL_EPS = 1e-3     # of a cell
FACE_EPS = 1e-5
MAX_LEFT_OUT = 0.02
MAX_ZEROED = 0.05

TRIPLANE_C16 = grid_sizes_for((2, 6, 5, 7, 16), True)
#   name: grid sizes, (R, N), grid form, contract, mask, half-width of the cube the points are drawn from
CASES = {
    "triplane_c16": (TRIPLANE_C16, (7, 37), "list", False, False, 1.2),
    "voxel_c32_flat": ([[2, 4, 3, 5, 32]], (7, 37), "flat", False, False, 1.2),
    "voxel_c5_mask": ([[2, 4, 3, 5, 5]], (7, 37), "list", False, True, 1.2),
    "triplane_c20_contract_mask": (grid_sizes_for((1, 8, 7, 9, 20), True), (7, 37), "list", True, True, 3.0),
    "voxel_c128": ([[1, 3, 4, 3, 128]], (3, 70), "list", False, False, 1.2),
    "mixed_list_c16": ([[2, 4, 3, 5, 16], [2, 1, 6, 7, 16], [2, 5, 1, 8, 16], [2, 6, 5, 1, 16]], (7, 37), "list", False, False, 1.2),
    "one_point": (TRIPLANE_C16, (1, 1), "list", False, False, 1.2),
    "one_wave": ([[1, 4, 3, 5, 16]], (1, 64), "list", False, False, 1.2),
    "one_cell": ([[1, 4, 3, 5, 32]], (1, 64), "list", False, False, None),  # every point inside cell (1, 1, 1)
}
SEEDS = {name: 500 + i for i, name in enumerate(CASES)}
INT32_IDX = "voxel_c32_flat"  # ray_grid_idx is int64 everywhere else
_CACHE = {}


def _unnorm(c, size):
    return ((c + 1) * size - 1) / 2


def _near_int(t, eps):
    return (t - torch.round(t)).abs() < eps


def bilinear_form(grids, points, gidx, vectors, mask, contract):
    """B(G, P, U) in the dtype of its arguments"""
    q = O.contract_pi(points) if contract else points
    return (O.sample_grid_list(grids, q, gidx, mask) * vectors).sum()


def case(name):
    if name in _CACHE:
        return _CACHE[name]
    sizes, (R, N), form, contract, mask, half = CASES[name]
    gen = torch.Generator().manual_seed(SEEDS[name])
    B, C = sizes[0][0], sizes[0][4]
    grids = [0.5 * torch.randn(s, generator=gen) for s in sizes]
    up_grids = [torch.randn(s, generator=gen) for s in sizes]      # upstream gradient of a splat
    if half is None:  # un-normalised coordinates in [1.1, 1.9] on every axis: one cell, away from its faces
        _, D, H, W, _ = sizes[0]
        t = 1.1 + 0.8 * torch.rand(R, N, 3, generator=gen)
        pts = (2 * t + 1) / torch.tensor([W, H, D], dtype=torch.float32) - 1
    else:
        pts = (torch.rand(R, N, 3, generator=gen) * 2 - 1) * half
    gidx = torch.randint(0, B, (R,), generator=gen)
    if name == INT32_IDX:
        gidx = gidx.to(torch.int32)
    vec = torch.randn(R, N, C, generator=gen)  # upstream gradient of the gather = features of the splat

    # ---- where fp32 geometry may take another branch (fp64 coordinates of the fp32 points) ----
    p64 = pts.double()
    q64 = O.contract_pi(p64) if contract else p64
    left_out = torch.zeros(R, N, dtype=torch.bool)
    if mask:
        left_out |= ((q64.abs() - 1.0).abs() < FACE_EPS).any(-1)
    on_face = torch.zeros(R, N, dtype=torch.bool)
    for s in sizes:
        for ax, size in ((0, s[3]), (1, s[2]), (2, s[1])):
            if size > 1:
                on_face |= _near_int(_unnorm(q64[..., ax], size), CELL_EPS)
    on_kink = torch.zeros(R, N, dtype=torch.bool)
    if contract:
        a = p64.abs().sort(dim=-1, descending=True).values
        on_kink = ((a[..., 0] - 1.0).abs() < CELL_EPS) | ((a[..., 0] > 1.0) & ((a[..., 0] - a[..., 1]) < CELL_EPS))
    zeroed = on_face | on_kink | left_out
    vec_kept = vec * (~left_out).float()[..., None]   # splat values
    vec_live = vec * (~zeroed).float()[..., None]     # point gradients

    # ---- fp64 oracle ----
    g64 = [g.double() for g in grids]
    u64 = [g.double() for g in up_grids]
    gather = O.sample_grid_list(g64, q64, gidx, mask)
    gather_up = O.sample_grid_list(u64, q64, gidx, mask)

    def d_grids(vectors, channels):
        leaves = [torch.zeros(s[:4] + [channels], dtype=torch.float64, requires_grad=True) for s in sizes]
        bilinear_form(leaves, p64, gidx, vectors, mask, contract).backward()
        return [t.grad for t in leaves]

    def d_points(gs, vectors):
        p = p64.clone().requires_grad_(True)
        bilinear_form(gs, p, gidx, vectors, mask, contract).backward()
        return p.grad

    d_grid = d_grids(vec.double(), C)              # the gather's grid gradient = the raw splat of `vec`
    splat_raw = d_grids(vec_kept.double(), C)
    weights = d_grids(torch.ones(R, N, 1, dtype=torch.float64), 1)
    splat_norm = [f / w.clamp(min=1e-5) for f, w in zip(splat_raw, weights)]
    gather_up_norm = O.sample_grid_list([u / w.clamp(min=1e-5) for u, w in zip(u64, weights)], q64, gidx, mask)
    _CACHE[name] = dict(name=name, sizes=sizes, grids=grids, up_grids=up_grids, pts=pts, gidx=gidx, vec=vec, vec_kept=vec_kept,
                        vec_live=vec_live, form=form, contract=contract, mask=mask, left_out=left_out, zeroed=zeroed,
                        counts=dict(on_face=int(on_face.sum()), on_kink=int(on_kink.sum()), left_out=int(left_out.sum())),
                        inside=O.in_bounds(q64), gather=gather, d_grid=d_grid, d_points_gather=d_points(g64, vec_live.double()),
                        splat_raw=splat_raw, weights=weights, splat_norm=splat_norm, gather_up=gather_up,
                        gather_up_norm=gather_up_norm, d_points_splat=d_points(u64, vec_live.double()))
    return _CACHE[name]


def grid_arg(c, grids, dev, requires_grad=False):
    """``grids`` on ``dev`` in the case's grid form: ``(list of tensors, None)`` or ``(flat tensor, sizes)``"""
    if c["form"] == "flat":
        C = grids[0].shape[-1]
        flat = torch.cat([g.reshape(-1, C) for g in grids]).to(dev)
        return (flat.requires_grad_(True) if requires_grad else flat), [list(g.shape) for g in grids]
    return [g.to(dev).requires_grad_(True) if requires_grad else g.to(dev) for g in grids], None


def in_form(c, grids):
    """oracle grids in the case's grid form, as a list of tensors (the flat tensor as a one-entry list)"""
    if c["form"] == "flat":
        C = grids[0].shape[-1]
        return [torch.cat([g.reshape(-1, C) for g in grids])]
    return list(grids)

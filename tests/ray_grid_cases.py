"""Inputs and fp64 oracle of the weighted splat / gather along rays (tests/test_ray_grid_host.py checks the inputs without a GPU,
tests/test_gpu_ray_grid.py holds the kernels to the oracle).  Every case is built once per process and never modified.

Oracle, in fp64 on the fp32 inputs, with ``p_rs = depths[r, s] * directions[r] + origins[r]`` and ``q = contract_pi(p)`` when asked:

    T(G, W, F; P) = sum(sample_grid_list(G, q, grid_idx, mask) * W[..., None] * F[:, None, :])

Every result is ``T`` itself or an autograd derivative of it: the raw splat ``dT/dG``, the gather ``dT/dF``, ``dT/dW``, ``dT/d depths``; the
normalised splat is ``F_sum / clamp(W_sum, 1e-5)`` with ``W_sum`` the raw splat of a one-channel ``F = 1``.

The interpolation weights are continuous across cell faces and across the kink of the contraction, so values and ``dT/dW`` need no
exclusions there.  Treated specially (the rules and caps of tests/point_grid_cases.py):
* with the mask only, samples within 1e-5 of a face of [-1, 1]^3 after the contraction (fp32 geometry may put them on the other side)
  have their WEIGHT zeroed (``w_kept``; their entry of ``dT/dW`` is not compared).  At most 2 % of a case; the cases with the mask that
  are normalised are seeded to have none at all.
* for the DEPTH gradient only, samples within 1e-3 of a cell of a cell face of any grid (the weights have a kink) or within 1e-3 of the
  kink of the contraction, and the samples above, have their weight zeroed (``w_live``: the depth gradient is linear in the sample's
  weight, so such a sample has none in the kernel and in the oracle alike).  At most 5 % of a case.
A seed that misses a cap is changed, never the cap.
"""
import torch

from oracle import lightplane_oracle as O
from tests.point_grid_cases import CELL_EPS, FACE_EPS, MAX_LEFT_OUT, MAX_ZEROED, TOL, TRIPLANE_C16, _near_int, _unnorm, grid_arg, in_form  # noqa: F401
from tests.synth import grid_sizes_for

DENSE_GRID = [[1, 4, 3, 16, 16]]
#   name: grid sizes, (R, S), grid form, contract, mask, rays ("random": half-width of the cube the rays cross | a scripted kind), weights
CASES = {
    "triplane_c16": (TRIPLANE_C16, (7, 37), "list", False, False, 1.2, "pos"),
    "voxel_c32_flat": ([[2, 4, 3, 5, 32]], (5, 70), "flat", False, False, 1.2, "pos"),
    "voxel_c5_mask": ([[2, 4, 3, 5, 5]], (7, 37), "list", False, True, 1.2, "pos"),
    "triplane_c20_contract_mask": (grid_sizes_for((1, 8, 7, 9, 20), True), (7, 37), "list", True, True, 3.0, "pos"),
    "voxel_c128": ([[1, 3, 4, 3, 128]], (5, 3), "list", False, False, 1.2, "pos"),
    "mixed_list_c16": ([[2, 4, 3, 5, 16], [2, 1, 6, 7, 16], [2, 5, 1, 8, 16], [2, 6, 5, 1, 16]], (7, 37), "list", False, False, 1.2, "pos"),
    "one_sample": (TRIPLANE_C16, (1, 1), "list", False, False, 0.8, "pos"),
    "one_cell": ([[1, 4, 3, 5, 32]], (1, 70), "list", False, False, "one_cell", "pos"),  # every sample inside cell (1, 1, 1)
    "dense_ray": (DENSE_GRID, (2, 130), "list", False, False, "dense", "pos"),           # steps of a tenth of a cell along x
    "sparse_ray": (DENSE_GRID, (2, 12), "list", False, False, "sparse", "pos"),          # steps of 1.3 cells along x
    "unsorted": (TRIPLANE_C16, (7, 37), "list", False, False, "unsorted", "pos"),         # depths in random order
    "signed_weights": ([[2, 4, 3, 5, 16]], (7, 37), "list", False, False, 1.2, "signed"),  # zero and negative weights: raw splat only
}
SEEDS = {name: 700 + i for i, name in enumerate(CASES)}
INT32_IDX = "voxel_c32_flat"  # rays.grid_idx is int64 everywhere else
_CACHE = {}


def form_t(grids, origins, directions, gidx, depths, weights, vec, mask, contract):
    """T(G, W, F; P) in the dtype of its arguments"""
    p = depths[..., None] * directions[:, None, :] + origins[:, None, :]
    q = O.contract_pi(p) if contract else p
    return (O.sample_grid_list(grids, q, gidx, mask) * weights[..., None] * vec[:, None, :]).sum()


def _scripted_rays(kind, sizes, R, S, gen):
    """(origins, directions, depths) of the scripted cases, through un-normalised coordinates t of the grid: c = (2 t + 1) / size - 1"""
    _, D, H, W, _ = sizes[0]
    size = torch.tensor([W, H, D], dtype=torch.float32)
    if kind == "one_cell":  # t in [1.1, 1.9] on every axis: one cell, away from its faces
        t0 = 1.1 + 0.3 * torch.rand(R, 3, generator=gen)
        t1 = 1.6 + 0.3 * torch.rand(R, 3, generator=gen)
        depths = torch.rand(R, S, generator=gen).sort(dim=1).values
    else:
        step = 0.1 if kind == "dense" else 1.3
        t0 = torch.tensor([0.55, 0.3, 0.4]) + 0.2 * torch.rand(R, 3, generator=gen)
        slope = torch.cat([torch.full((R, 1), step), step * 0.11 * torch.rand(R, 2, generator=gen)], dim=1)
        t1 = t0 + slope  # (one depth unit = one step)
        depths = torch.arange(S, dtype=torch.float32).expand(R, S).clone()
    o = (2 * t0 + 1) / size - 1
    d = (2 * t1 + 1) / size - 1 - o
    return o, d, depths


def case(name):
    if name in _CACHE:
        return _CACHE[name]
    sizes, (R, S), form, contract, mask, rays, wkind = CASES[name]
    gen = torch.Generator().manual_seed(SEEDS[name])
    B, C = sizes[0][0], sizes[0][4]
    grids = [0.5 * torch.randn(s, generator=gen) for s in sizes]
    up_grids = [torch.randn(s, generator=gen) for s in sizes]  # upstream gradient of a splat
    if isinstance(rays, str) and rays != "unsorted":
        origins, directions, depths = _scripted_rays(rays, sizes, R, S, gen)
    else:  # a ray from one random point of the cube to another; depths a little beyond both ends
        half = 1.2 if rays == "unsorted" else rays
        a = (torch.rand(R, 3, generator=gen) * 2 - 1) * half
        b = (torch.rand(R, 3, generator=gen) * 2 - 1) * half
        origins, directions = a, b - a
        depths = (torch.rand(R, S, generator=gen) * 1.2 - 0.1).sort(dim=1).values
        if rays == "unsorted":
            depths = torch.gather(depths, 1, torch.rand(R, S, generator=gen).argsort(dim=1))
    gidx = torch.randint(0, B, (R,), generator=gen)
    if name == INT32_IDX:
        gidx = gidx.to(torch.int32)
    if wkind == "pos":
        weights = 0.1 + torch.rand(R, S, generator=gen)
    else:  # a third exactly zero, the others of either sign
        weights = torch.randn(R, S, generator=gen) * (torch.rand(R, S, generator=gen) > 1 / 3).float()
    feat = torch.randn(R, C, generator=gen)   # the splat's per-ray feature
    g_out = torch.randn(R, C, generator=gen)  # upstream gradient of the gather

    # ---- where fp32 geometry may take another branch (fp64 coordinates of the fp32 inputs) ----
    o64, d64, t64 = origins.double(), directions.double(), depths.double()
    p64 = t64[..., None] * d64[:, None, :] + o64[:, None, :]
    q64 = O.contract_pi(p64) if contract else p64
    left_out = torch.zeros(R, S, dtype=torch.bool)
    if mask:
        left_out |= ((q64.abs() - 1.0).abs() < FACE_EPS).any(-1)
    on_face = torch.zeros(R, S, dtype=torch.bool)
    for s in sizes:
        for ax, size in ((0, s[3]), (1, s[2]), (2, s[1])):
            if size > 1:
                on_face |= _near_int(_unnorm(q64[..., ax], size), CELL_EPS)
    on_kink = torch.zeros(R, S, dtype=torch.bool)
    if contract:
        a = p64.abs().sort(dim=-1, descending=True).values
        on_kink = ((a[..., 0] - 1.0).abs() < CELL_EPS) | ((a[..., 0] > 1.0) & ((a[..., 0] - a[..., 1]) < CELL_EPS))
    zeroed = on_face | on_kink | left_out
    w_kept = weights * (~left_out).float()  # values and every gradient but the depths'
    w_live = weights * (~zeroed).float()    # depth gradients

    # ---- fp64 oracle ----
    g64 = [g.double() for g in grids]
    u64 = [g.double() for g in up_grids]

    def T(gs, w, vec, t=t64):
        return form_t(gs, o64, d64, gidx, t, w, vec, mask, contract)

    def d_grids(w, vec):
        leaves = [torch.zeros(s[:4] + [vec.shape[1]], dtype=torch.float64, requires_grad=True) for s in sizes]
        T(leaves, w, vec).backward()
        return [t.grad for t in leaves]

    def d_vec(gs, w):
        v = torch.zeros(R, C, dtype=torch.float64, requires_grad=True)
        T(gs, w, v).backward()
        return v.grad

    def d_weights(gs, vec):
        w = torch.zeros(R, S, dtype=torch.float64, requires_grad=True)
        T(gs, w, vec).backward()
        return w.grad

    def d_depths(gs, w, vec):
        t = t64.clone().requires_grad_(True)
        T(gs, w, vec, t).backward()
        return t.grad

    wk, wl, f64, go64 = w_kept.double(), w_live.double(), feat.double(), g_out.double()
    splat_raw = d_grids(wk, f64)
    w_sum = d_grids(wk, torch.ones(R, 1, dtype=torch.float64))
    splat_norm = [f / w.clamp(min=1e-5) for f, w in zip(splat_raw, w_sum)]
    _CACHE[name] = dict(
        name=name, sizes=sizes, grids=grids, up_grids=up_grids, origins=origins, directions=directions, depths=depths, gidx=gidx,
        weights=weights, w_kept=w_kept, w_live=w_live, feat=feat, g_out=g_out, form=form, contract=contract, mask=mask,
        normalize=wkind == "pos", left_out=left_out, zeroed=zeroed,
        counts=dict(on_face=int(on_face.sum()), on_kink=int(on_kink.sum()), left_out=int(left_out.sum())),
        inside=O.in_bounds(q64), q64=q64,
        # the splat and its gradients (upstream up_grids)
        splat_raw=splat_raw, w_sum=w_sum, splat_norm=splat_norm,
        splat_d_feat=d_vec(u64, wk), splat_d_feat_norm=d_vec([u / w.clamp(min=1e-5) for u, w in zip(u64, w_sum)], wk),
        splat_d_weights=d_weights(u64, f64), splat_d_depths=d_depths(u64, wl, f64),
        # the gather and its gradients (upstream g_out)
        gather=d_vec(g64, wk), gather_d_grid=d_grids(wk, go64), gather_d_weights=d_weights(g64, go64),
        gather_d_depths=d_depths(g64, wl, go64))
    return _CACHE[name]

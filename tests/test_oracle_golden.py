"""Pin the CPU oracle (oracle/lightplane_oracle.py) against fixtures produced by the
reference's own naive implementation (tests/golden/make_golden.py).  CPU only.

Tolerance: the oracle is a re-statement with a different (but mathematically
identical) operation order (explicit gathers instead of F.grid_sample, scatter via
index_add), so agreement is at fp32 round-off: 2e-5 relative to the tensor scale.
"""
import os

import numpy as np
import pytest
import torch

from oracle import lightplane_oracle as O
from tests.synth import RENDERER_CASES, SPLATTER_CASES

REL_TOL = 2e-5


def _close(name, got, want, tol=REL_TOL):
    got = torch.as_tensor(got, dtype=torch.float64)
    want = torch.as_tensor(np.asarray(want), dtype=torch.float64)
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    scale = max(want.abs().max().item(), 1e-6)
    err = (got - want).abs().max().item() / scale
    assert err <= tol, f"{name}: max err / scale = {err:.3e} > {tol}"


def _check_inputs(d, z):
    r = d["rays"]
    for k in ("directions", "origins", "near", "far", "encoding"):
        assert np.array_equal(getattr(r, k).numpy(), z[k]), f"seeded input {k} drifted from the golden file"
    assert np.array_equal(r.grid_idx.numpy(), z["grid_idx"])


@pytest.mark.parametrize("case", RENDERER_CASES, ids=lambda c: c.name)
def test_renderer_oracle_matches_reference(case, golden_dir):
    z = np.load(os.path.join(golden_dir, f"renderer__{case.name}.npz"))
    d = case.build()
    _check_inputs(d, z)
    assert np.array_equal(d["decoder"].mlp_params.numpy(), z["mlp_params"])
    rays, dec = d["rays"], d["decoder"]
    rays.encoding = rays.encoding.clone().requires_grad_(True)
    dec.mlp_params = dec.mlp_params.clone().requires_grad_(True)
    grids = [g.clone().requires_grad_(True) for g in d["grids"]]
    cgrids = None if d["color_grids"] is None else [g.clone().requires_grad_(True) for g in d["color_grids"]]
    out = O.lightplane_renderer_naive(rays, grids, dec, scaffold=d["scaffold"], color_grid=cgrids, **d["cfg"])
    _close("ray_length", out[0].detach(), z["ray_length"])
    _close("neg_log_t", out[1].detach(), z["neg_log_t"])
    _close("feature", out[2].detach(), z["feature"])
    g_len, g_nlt, g_feat = d["upstream"]
    ((out[0] * g_len).sum() + (out[1] * g_nlt).sum() + (out[2] * g_feat).sum()).backward()
    _close("grad_mlp_params", dec.mlp_params.grad, z["grad_mlp_params"])
    _close("grad_encoding", rays.encoding.grad, z["grad_encoding"])
    for i, g in enumerate(grids):
        _close(f"grad_grid{i}", g.grad, z[f"grad_grid{i}"])
    if cgrids is not None:
        for i, g in enumerate(cgrids):
            _close(f"grad_cgrid{i}", g.grad, z[f"grad_cgrid{i}"])


@pytest.mark.parametrize("case", SPLATTER_CASES, ids=lambda c: c.name)
def test_splatter_oracle_matches_reference(case, golden_dir):
    z = np.load(os.path.join(golden_dir, f"splatter__{case.name}.npz"))
    d = case.build()
    _check_inputs(d, z)
    rays = d["rays"]
    rays.encoding = rays.encoding.clone().requires_grad_(True)
    if d["mlp"] is None:
        out = O.lightplane_splatter_naive(rays, d["out_sizes"], **d["cfg"])
        in_grids = None
    else:
        d["mlp"].mlp_params = d["mlp"].mlp_params.clone().requires_grad_(True)
        in_grids = [g.clone().requires_grad_(True) for g in d["in_grids"]]
        out = O.lightplane_mlp_splatter_naive(rays, d["out_sizes"], d["mlp"], in_grids, **d["cfg"])
    for i, o in enumerate(out):
        _close(f"out{i}", o.detach(), z[f"out{i}"])
    sum((o * u).sum() for o, u in zip(out, d["upstream"])).backward()
    _close("grad_encoding", rays.encoding.grad, z["grad_encoding"])
    if in_grids is not None:
        _close("grad_mlp_params", d["mlp"].mlp_params.grad, z["grad_mlp_params"])
        for i, g in enumerate(in_grids):
            _close(f"grad_in_grid{i}", g.grad, z[f"grad_in_grid{i}"])


def test_baseline_cfg1_oracle_matches_reference(golden_dir):
    """BASELINE.json configs[0] exactly (1 000 random rays, voxel 32^3 x 16, 64 samples, 2/2/2 x 32): the oracle against
    the outputs / gradients the reference's naive renderer produced for it (tests/golden/make_golden.py baseline_cfg1)."""
    from tests.synth import baseline_cfg1
    z = np.load(os.path.join(golden_dir, "renderer__baseline_cfg1.npz"))
    d = baseline_cfg1()
    rays, dec = d["rays"], d["decoder"]
    sums = [d["grids"][0].double().sum().item(), rays.directions.double().sum().item(), rays.encoding.double().sum().item(),
            dec.mlp_params.double().sum().item()]
    assert np.allclose(sums, z["checksum_inputs"], rtol=0, atol=1e-9), "seeded inputs drifted from the golden file"
    rays.encoding = rays.encoding.clone().requires_grad_(True)
    dec.mlp_params = dec.mlp_params.clone().requires_grad_(True)
    grids = [g.clone().requires_grad_(True) for g in d["grids"]]
    out = O.lightplane_renderer_naive(rays, grids, dec, **d["cfg"])
    g_len, g_nlt, g_feat = d["upstream"]
    ((out[0] * g_len).sum() + (out[1] * g_nlt).sum() + (out[2] * g_feat).sum()).backward()
    for nm, a in (("ray_length", out[0]), ("neg_log_t", out[1]), ("feature", out[2]), ("grad_mlp_params", dec.mlp_params.grad),
                  ("grad_encoding", rays.encoding.grad), ("grad_grid0", grids[0].grad)):
        _close(nm, a.detach(), z[nm])


def test_hash_rng_matches_reference(golden_dir):
    z = np.load(os.path.join(golden_dir, "randn.npz"))
    x1, x2 = torch.from_numpy(z["x1"]), torch.from_numpy(z["x2"])
    for seed in (0, 5, 123456):
        got = O.int_to_randn(x1, x2, seed)
        assert np.array_equal(got.numpy(), z[f"z_seed{seed}"]), f"seed {seed}: RNG not bit-identical"


def test_oracle_fp64_close_to_fp32():
    """The oracle runs in fp64 too (tighter reference for the HIP tolerance budget)."""
    d = RENDERER_CASES[1].build()
    rays, dec = d["rays"], d["decoder"]
    out32 = O.lightplane_renderer_naive(rays, d["grids"], dec, **d["cfg"])
    import copy
    r64 = copy.copy(rays)
    for k in ("directions", "origins", "near", "far", "encoding"):
        setattr(r64, k, getattr(rays, k).double())
    dec64 = copy.copy(dec)
    dec64.mlp_params = dec.mlp_params.double()
    out64 = O.lightplane_renderer_naive(r64, [g.double() for g in d["grids"]], dec64, **d["cfg"])
    for a, b in zip(out32, out64):
        _close("fp32-vs-fp64", a, b, tol=1e-5)


def test_geometry_dtype_keeps_the_references_cells_and_weights():
    """oracle.geometry_dtype(fp32) under an fp64 run: the same cells / interpolation weights as the fp32 oracle (the geometry the
    reference defines), a wide decoder on top -- outputs within fp32 round-off of both, and no effect outside the context."""
    import copy
    d = next(c for c in RENDERER_CASES if c.name == "voxel_inf_contract").build() if any(c.name == "voxel_inf_contract" for c in RENDERER_CASES) else RENDERER_CASES[0].build()

    def run(dtype, geom=None):
        r = copy.copy(d["rays"])
        for f in ("directions", "origins", "near", "far", "encoding"):
            setattr(r, f, getattr(r, f).to(dtype))
        dec = copy.copy(d["decoder"])
        dec.mlp_params = dec.mlp_params.to(dtype)
        g = [x.to(dtype) for x in d["grids"]]
        cg = None if d["color_grids"] is None else [x.to(dtype) for x in d["color_grids"]]
        sc = None if d["scaffold"] is None else d["scaffold"].to(dtype)
        if geom is None:
            return O.lightplane_renderer_naive(r, g, dec, scaffold=sc, color_grid=cg, **d["cfg"])
        with O.geometry_dtype(geom):
            return O.lightplane_renderer_naive(r, g, dec, scaffold=sc, color_grid=cg, **d["cfg"])

    a32, a64, mixed, again = run(torch.float32), run(torch.float64), run(torch.float64, torch.float32), run(torch.float64)
    for x32, x64, xm, xa in zip(a32, a64, mixed, again):
        assert xm.dtype == torch.float64 and torch.equal(x64, xa)
        scale = float(x64.abs().max())
        assert float((xm - x64).abs().max()) / scale < 2e-5 and float((xm - x32.double()).abs().max()) / scale < 2e-5
    assert O._GEOMETRY_DTYPE is None


def test_near_tie_masks_contain_every_fp32_vs_fp64_relu_flip():
    """The theory behind the GPU suite's tie masks (tests/test_gpu_parity.py TieMasks), checked on flips that are certainly
    flips: the oracle in fp32 against the same oracle in fp64 on a whole pinhole image.  Every `grad_grid` / `grad_encoding`
    entry on which the two disagree by more than the 1e-4 bar must lie where a sample with a near-zero ReLU pre-activation
    reaches (its tap rows, its ray) -- and the masks must be informative (cover well under all of the tensor)."""
    from tests.test_gpu_coherent import coherent_renderer_inputs, oracle_renderer64
    from tests.test_gpu_parity import TieMasks, run_oracle_renderer

    d = coherent_renderer_inputs("triplane_plus_voxel_c16", "64x64_axis")
    o32 = run_oracle_renderer(d)
    o64 = oracle_renderer64(d)
    ties = TieMasks(d)
    n_flipped = 0
    for i, (a, b) in enumerate(zip(o32[3], o64[3])):
        scale = float(b.abs().max())
        off = ((a.double() - b).abs() / scale) > 1e-4
        mask = ties.grid_mask(i)().expand_as(off)
        assert not bool((off & ~mask).any()), f"grid {i}: {int((off & ~mask).sum())} flipped entries outside the near-tie mask"
        assert float(mask.float().mean()) < 0.6, f"grid {i}: the mask covers {float(mask.float().mean()):.2f} of the rows -- it says nothing"
        n_flipped += int(off.sum())
    off = ((o32[2].double() - o64[2]).abs() / float(o64[2].abs().max())) > 1e-4
    mask = ties.encoding_mask()().expand_as(off)
    assert not bool((off & ~mask).any()) and float(mask.float().mean()) < 0.1
    assert n_flipped > 100, "this case is known to carry a few hundred flipped entries: the test would be vacuous without them"


def test_chunked_splatter_oracle_equals_oracle():
    """tests/test_gpu_config_scale.py evaluates the Splatter oracle in ray chunks for BASELINE configs[2] at full size (65 536
    rays x 256 samples do not fit `lightplane_splatter_naive`'s [N, S, C] tensors); the chunked form is the oracle's own corner
    arithmetic and must equal the oracle + autograd on a case small enough for both."""
    from tests.synth import pinhole_rays
    from tests.test_gpu_config_scale import splatter_oracle_chunked

    gen = torch.Generator().manual_seed(5)
    for mask in (True, False):
        rays = pinhole_rays(24, 40, cam_dist=2.3, azimuth_deg=20.0, elevation_deg=35.0)
        rays.encoding = torch.rand(rays.n_rays, 32, generator=gen).requires_grad_(True)
        shape = [1, 12, 14, 10, 32]
        cfg = dict(num_samples=20, num_samples_inf=0, mask_out_of_bounds_samples=mask, contract_coords=False)
        up = torch.randn(*shape, generator=gen)
        (want,) = O.lightplane_splatter_naive(rays, [shape], **cfg)
        (want * up).sum().backward()
        with torch.no_grad():
            got, g_enc, wgrid = splatter_oracle_chunked(rays, shape, cfg, up, chunk=100)
        _close("chunked oracle: out", got, want.detach().numpy(), tol=2e-6)
        _close("chunked oracle: grad_encoding", g_enc, rays.encoding.grad.numpy(), tol=2e-6)
        assert torch.equal(wgrid > 0, (want.detach() != 0).any(dim=-1))


def test_chunked_mlp_splatter_oracle_equals_oracle():
    """oracle.lightplane_mlp_splatter_chunked (the fp64 MLP-Splatter oracle of the GPU suite's forced proofs at full-chip batches: the
    weight grid once from the geometry, then forward + backward per ray chunk) equals lightplane_mlp_splatter_naive + autograd in fp64
    -- outputs and every gradient -- for several chunk sizes, with and without the out-of-bounds mask; and geometry_dtype(fp32) keeps
    the fp32 oracle's cells and weights under fp64 features."""
    import copy
    from tests.synth import SplatterCase

    F64 = torch.float64
    for mask in (True, False):
        case = SplatterCase("chunked", seed=31, n_rays=70, out_base=(2, 7, 5, 6, 16), is_triplane=not mask, num_samples=13,
                            num_samples_inf=2, mask_oob=mask, contract=not mask, use_mlp=True, n_layers=3, hidden=32, feat_dim=16,
                            in_base=(2, 5, 4, 6, 16), in_triplane=mask)
        d = case.build()
        rays = copy.copy(d["rays"])
        for f in ("directions", "origins", "near", "far", "encoding"):
            setattr(rays, f, getattr(rays, f).to(F64))
        mlp = copy.copy(d["mlp"])
        mlp.mlp_params = d["mlp"].mlp_params.to(F64)
        in_grids = [g.to(F64) for g in d["in_grids"]]
        up = [u.to(F64) for u in d["upstream"]]

        r = copy.copy(rays)
        r.encoding = r.encoding.clone().requires_grad_(True)
        m = copy.copy(mlp)
        m.mlp_params = mlp.mlp_params.clone().requires_grad_(True)
        g = [x.clone().requires_grad_(True) for x in in_grids]
        want = O.lightplane_mlp_splatter_naive(r, d["out_sizes"], m, g, **d["cfg"])
        sum((o * u).sum() for o, u in zip(want, up)).backward()
        for chunk in (1, 16, 33, 70, 1000):
            outs, g_enc, g_par, g_in = O.lightplane_mlp_splatter_chunked(rays, d["out_sizes"], mlp, in_grids, up, chunk=chunk, **d["cfg"])
            assert g_enc.dtype == F64 and g_par.dtype == F64
            for k, (a, b) in enumerate(zip(outs, want)):
                _close(f"chunk {chunk}: out{k}", a, b.detach().numpy(), tol=1e-12)
            _close(f"chunk {chunk}: grad_encoding", g_enc, r.encoding.grad.numpy(), tol=1e-12)
            _close(f"chunk {chunk}: grad_mlp_params", g_par, m.mlp_params.grad.numpy(), tol=1e-12)
            for k, (a, b) in enumerate(zip(g_in, g)):
                _close(f"chunk {chunk}: grad_input_grid{k}", a, b.grad.numpy(), tol=1e-12)

        # geometry_dtype: fp64 features on the fp32 geometry are within fp32 round-off of both oracles, and the dtype reverts
        r32 = copy.copy(d["rays"])
        m32 = copy.copy(d["mlp"])
        o32 = O.lightplane_mlp_splatter_naive(r32, d["out_sizes"], m32, d["in_grids"], **d["cfg"])
        with O.geometry_dtype(torch.float32):
            mixed = O.lightplane_mlp_splatter_naive(rays, d["out_sizes"], mlp, in_grids, **d["cfg"])
        assert O._GEOMETRY_DTYPE is None
        for a32, a64, am in zip(o32, want, mixed):
            assert am.dtype == F64
            scale = float(a64.detach().abs().max())
            assert float((am - a64.detach()).abs().max()) / scale < 2e-5 and float((am - a32.double()).abs().max()) / scale < 2e-5


# ---------------------------------------------------------------------------------------------------------------------
# the box-restricted Splatter oracle (oracle.splatter_box_oracle) and the in-place weight pass (oracle.splatter_weight_grids): the
# references of tests/test_gpu_config_scale.py::test_cfg5_full_chain_against_oracle, equal to the full oracle where both run
# ---------------------------------------------------------------------------------------------------------------------
BOX_SHAPE = [1, 12, 14, 10, 8]   # [B, D, H, W, C]: D, H, W all different, so a transposed axis cannot pass
BOX_S = 24


def _box_rays():
    """Rays of every kind the prefilter has to get right: a pinhole image from outside (rays that cross the grid obliquely, rays that
    miss it), rays parallel to each axis (both directions) on a lattice of un-normalised coordinates at, just inside and just outside
    every integer -- a face of the footprint region of some box lies on each --, rays that start inside the grid, rays far away."""
    import math as _m
    from lightplane_amd.rays import Rays
    from tests.synth import cat_rays, pinhole_rays
    gen = torch.Generator().manual_seed(17)
    _, D, H, W, C = BOX_SHAPE
    size = {0: W, 1: H, 2: D}
    parts = [pinhole_rays(16, 20, cam_dist=2.3, azimuth_deg=20.0, elevation_deg=35.0)]
    for ax in (0, 1, 2):
        a, b = [q for q in (0, 1, 2) if q != ax]
        ua = torch.tensor([-1.0, -0.9999, 0.0, 2.0, 3.0001, 4.5, size[a] - 1.0, size[a] - 0.5, float(size[a])])
        ub = torch.tensor([-1.0, 1.0, 2.9999, 5.0, size[b] - 1.0, float(size[b])])
        uu_a, uu_b = torch.meshgrid(ua, ub, indexing="ij")
        n = uu_a.numel()
        o = torch.zeros(n, 3)
        o[:, a] = (uu_a.reshape(-1) + 0.5) * 2.0 / size[a] - 1.0
        o[:, b] = (uu_b.reshape(-1) + 0.5) * 2.0 / size[b] - 1.0
        for sign in (1.0, -1.0):
            oo = o.clone()
            oo[:, ax] = -2.0 * sign
            dd = torch.zeros(n, 3)
            dd[:, ax] = sign
            parts.append(Rays(directions=dd, origins=oo, grid_idx=torch.zeros(n, dtype=torch.long), near=torch.full((n,), 0.7),
                              far=torch.full((n,), 3.3), encoding=None))
    n = 200   # starting inside the grid (and inside most boxes), random directions, short marches
    dd = torch.randn(n, 3, generator=gen)
    parts.append(Rays(directions=dd / dd.norm(dim=-1, keepdim=True), origins=torch.rand(n, 3, generator=gen) * 1.4 - 0.7,
                      grid_idx=torch.zeros(n, dtype=torch.long), near=torch.zeros(n), far=torch.full((n,), 1.3), encoding=None))
    n = 20    # far away and pointing away
    parts.append(Rays(directions=torch.ones(n, 3) / _m.sqrt(3.0), origins=torch.full((n, 3), 3.0) + torch.rand(n, 3, generator=gen),
                      grid_idx=torch.zeros(n, dtype=torch.long), near=torch.zeros(n), far=torch.full((n,), 2.0), encoding=None))
    rays = cat_rays(parts)
    rays.encoding = torch.rand(rays.n_rays, C, generator=gen)
    return rays


def _box_cases():
    """(name, ((z0, z1), (y0, y1), (x0, x1))): a box at each corner of the grid (every face and every corner, clamped and partly
    valid corners), a box on each face alone, one interior box, a single cell, the whole grid."""
    _, D, H, W, _ = BOX_SHAPE
    boxes = []
    for bits in range(8):
        z = (0, 5) if bits & 4 else (7, D)
        y = (0, 6) if bits & 2 else (9, H)
        x = (0, 4) if bits & 1 else (6, W)
        boxes.append((f"corner{bits}", (z, y, x)))
    mid = ((4, 8), (5, 10), (3, 7))
    for ax, ext in enumerate((D, H, W)):
        for lo, hi in ((0, 3), (ext - 3, ext)):
            b = list(mid)
            b[ax] = (lo, hi)
            boxes.append((f"face{ax}_{lo}", tuple(b)))
    boxes += [("interior", ((3, 9), (4, 10), (2, 8))), ("single_cell", ((6, 7), (7, 8), (4, 5))), ("whole", ((0, D), (0, H), (0, W)))]
    return boxes


def _rays64(rays):
    import copy
    r = copy.copy(rays)
    for f in ("directions", "origins", "near", "far", "encoding"):
        setattr(r, f, getattr(rays, f).to(torch.float64))
    return r


def _naive_box_reference(rays, cfg, box, gen):
    """The full fp64 oracle on the reference's fp32 geometry: normalised output, un-normalised feature / weight sums (the oracle's own
    scatter, oracle._splat_one_grid) and, for an upstream zero outside ``box``, grad_encoding by autograd."""
    B, D, H, W, C = BOX_SHAPE
    r = _rays64(rays)
    r.encoding = r.encoding.clone().requires_grad_(True)
    up = torch.zeros(D, H, W, C, dtype=torch.float64)
    (z0, z1), (y0, y1), (x0, x1) = box
    up[z0:z1, y0:y1, x0:x1] = torch.randn(z1 - z0, y1 - y0, x1 - x0, C, generator=gen, dtype=torch.float64)
    with O.geometry_dtype(torch.float32):
        (out,) = O.lightplane_splatter_naive(r, [BOX_SHAPE], num_samples=BOX_S, **cfg)
        (out[0] * up).sum().backward()
        pts = O._splatter_points(r, BOX_S, 0, False, 1e-5)
    mask = O.in_bounds(pts).double() if cfg["mask_out_of_bounds_samples"] else torch.ones(pts.shape[:-1], dtype=torch.float64)
    with torch.no_grad():
        f = O._splat_one_grid(torch.zeros(D * H * W, C, dtype=torch.float64), BOX_SHAPE, pts, r.grid_idx,
                              r.encoding[:, None, :].expand(-1, BOX_S, -1), mask)
        w = O._splat_one_grid(torch.zeros(D * H * W, 1, dtype=torch.float64), BOX_SHAPE, pts, r.grid_idx,
                              torch.ones(pts.shape[:-1] + (1,), dtype=torch.float64), mask)
    return out[0].detach(), f.reshape(D, H, W, C), w.reshape(D, H, W), up, r.encoding.grad


def _box_values(res):
    return res.feature_sums / res.weight_sums.clamp(min=1e-5)[..., None]


@pytest.mark.parametrize("mask", [False, True], ids=["nomask", "mask_oob"])
def test_box_splatter_oracle_equals_oracle(mask):
    """oracle.splatter_box_oracle (only the samples the analytic prefilter keeps, corners outside the box dropped) and the in-place
    fp64 weight pass equal lightplane_splatter_naive in fp64 on the fp32 geometry, restricted to the box, at the 2e-6 of
    test_chunked_splatter_oracle_equals_oracle: feature sums, weight sums, normalised values, and grad_encoding of every ray against
    autograd of the full oracle with an upstream zero outside the box.  Every box of _box_cases, all ray kinds of _box_rays.
    The bar bites: a splat with one sample per ray dropped and one with the rays moved by a quarter cell miss 1e-4 in the box."""
    B, D, H, W, C = BOX_SHAPE
    rays = _box_rays()
    cfg = dict(num_samples_inf=0, mask_out_of_bounds_samples=mask, contract_coords=False)
    gen = torch.Generator().manual_seed(3 + mask)
    (wpass,) = O.splatter_weight_grids(rays, [BOX_SHAPE], BOX_S, sum_dtype=torch.float64, chunk=97, **cfg)
    assert wpass.dtype == torch.float64
    wpass = wpass.reshape(D, H, W)
    seen_cand, seen_miss, seen_partial = 0, 0, 0
    for name, box in _box_cases():
        out, f, w, up, g_want = _naive_box_reference(rays, cfg, box, gen)
        (z0, z1), (y0, y1), (x0, x1) = box
        sel = (slice(z0, z1), slice(y0, y1), slice(x0, x1))
        res = O.splatter_box_oracle(rays, BOX_SHAPE, box, dict(cfg, num_samples=BOX_S), upstream=up)
        _close(f"{name}: feature sums", res.feature_sums, f[sel].numpy(), tol=2e-6)
        _close(f"{name}: weight sums", res.weight_sums, w[sel].numpy(), tol=2e-6)
        _close(f"{name}: weight pass", wpass[sel], w[sel].numpy(), tol=2e-6)
        _close(f"{name}: values", _box_values(res), out[sel].numpy(), tol=2e-6)
        _close(f"{name}: grad_encoding", res.grad_encoding, g_want.numpy(), tol=2e-6)
        assert bool((res.grad_encoding[~res.candidates] == 0).all())
        assert int((w[sel] > 0).sum()) > 0 and bool((g_want[~res.candidates] == 0).all())
        seen_cand += int(res.candidates.sum())
        seen_miss += int((~res.candidates).sum())
        seen_partial += int((res.n_samples < res.candidates.sum() * BOX_S))
    assert seen_cand > 0 and seen_miss > 0 and seen_partial > 0
    _close("weight pass, whole grid", wpass, w.numpy(), tol=2e-6)

    # the bar bites: subtly wrong splats of the same rays, through the same box oracle, miss 1e-4 inside the box
    box = dict(_box_cases())["interior"]
    ref =_box_values(O.splatter_box_oracle(rays, BOX_SHAPE, box, dict(cfg, num_samples=BOX_S)))
    import copy
    drop = copy.copy(rays)     # the first sample of every ray dropped: S - 1 samples from the second sample's depth on
    drop.near = rays.near + (rays.far - rays.near) / (BOX_S - 1)
    moved = copy.copy(rays)    # every ray moved by a quarter cell along x
    moved.origins = rays.origins + torch.tensor([0.25 * 2.0 / W, 0.0, 0.0])
    for nm, r, s in (("one sample dropped", drop, BOX_S - 1), ("moved a quarter cell", moved, BOX_S)):
        got = _box_values(O.splatter_box_oracle(r, BOX_SHAPE, box, dict(cfg, num_samples=s)))
        err = float((got - ref).abs().max() / ref.abs().max())
        assert err > 1e-4, f"{nm}: differs from the right splat by only {err:.2e}: the 1e-4 bar would not see it"


def test_box_splatter_oracle_refuses_what_it_does_not_cover():
    """Triplanes, contraction, beyond-far samples, several batch entries and empty boxes raise; they are never approximated."""
    rays = _box_rays()
    cfg = dict(num_samples=BOX_S, num_samples_inf=0, mask_out_of_bounds_samples=False, contract_coords=False)
    box = ((0, 2), (0, 2), (0, 2))
    with pytest.raises(NotImplementedError):
        O.splatter_box_oracle(rays, [1, 1, 14, 10, 8], box, cfg)
    with pytest.raises(NotImplementedError):
        O.splatter_box_oracle(rays, [2, 12, 14, 10, 8], box, cfg)
    with pytest.raises(NotImplementedError):
        O.splatter_box_oracle(rays, BOX_SHAPE, box, dict(cfg, contract_coords=True))
    with pytest.raises(NotImplementedError):
        O.splatter_box_oracle(rays, BOX_SHAPE, box, dict(cfg, num_samples_inf=4))
    with pytest.raises(ValueError):
        O.splatter_box_oracle(rays, BOX_SHAPE, ((3, 3), (0, 2), (0, 2)), cfg)
    up = torch.zeros(BOX_SHAPE)
    up[0, 5, 5, 5, 0] = 1.0
    with pytest.raises(AssertionError, match="outside the box"):
        O.splatter_box_oracle(rays, BOX_SHAPE, box, cfg, upstream=up)

"""GPU parity AT the BASELINE.json configurations (not at shrunk versions of them).

* configs[1] (cfg 2, the headline): ALL 65 536 rays of the 256 x 256 image on the 64^2 x 16 triplane at 128 samples -- the launch
  bench.py times -- outputs and all gradient families against the CPU oracle, which runs the batch in ray chunks and
  accumulates the gradients (fp32 = the reference's arithmetic, and fp64 to tell ReLU flips from errors).
* configs[0] (cfg 1) exactly: 1 000 random rays, voxel 32^3 x 16, 64 samples, against the oracle AND against
  tests/golden/renderer__baseline_cfg1.npz, the numbers the reference's naive renderer produced for it.
* the 1080p reporting batch: a REAL 1920 x 1080 launch (C = 16 at 128 samples, C = 32 at 64 samples) whose upstream gradient
  is non-zero on a 24 x 40 pixel block only -- every other ray then contributes exactly nothing, so the whole launch's grid /
  parameter gradients must equal the oracle's gradients of the block alone, and its outputs / encoding gradients on the block
  the oracle's (per-ray quantities; the rest of grad_encoding must be exactly zero).
* configs[2] (cfg 3): the whole 128^3 x 32 splat of 65 536 rays and their grad_encoding against the chunked oracle.
* configs[4] (cfg 5): one chained step of bench.py's JointWorkload at full size -- 13 views x 512^2 rays splatted into the 2.15 GB
  256^3 x 32 grid, 135 x 1920 rays rendered from it, the backward through the normalisation into every splat ray's encoding -- against
  the in-place fp64 weight pass over all 16.7 M cells, oracle.splatter_box_oracle on boxes of cells, and the forced fp64 Renderer proof.
* index parity from the HOT kernels: the set of grid rows the MFMA backward scatters into equals the oracle's, exactly
  (test_corner_indices_bit_exact proves the formulas on a debug kernel; this proves the production tap code -- axis_taps /
  triplane_taps with the border re-expression, the voxel column walk -- addresses the same cells).
"""
import copy
import math
import os

import numpy as np
import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib
from oracle import lightplane_oracle as O
from tests.synth import baseline_cfg1, cfg2_inputs, grid_sizes_for, pinhole_rays, random_decoder, random_grids
from tests.test_gpu_parity import _assert_close, _dev, assert_grad_close, forced_oracle_check, relu_site_widths, run_hip_renderer

pytestmark = pytest.mark.gpu
F64 = torch.float64


def oracle_chunked(d, idx=None, dtype=torch.float32, chunk=2048):
    """Oracle forward + backward over the rays ``idx`` (default: all) in chunks, gradients of the replicated inputs summed."""
    # (a problem of this size thrashes on the box's 100+ host cores: bench.py's cpu_baseline leg measured 16 threads as the knee)
    old_threads = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    try:
        return _oracle_chunked(d, idx, dtype, chunk)
    finally:
        torch.set_num_threads(old_threads)


def _oracle_chunked(d, idx, dtype, chunk):
    rays = d["rays"] if idx is None else d["rays"][idx]
    up = d["upstream"] if idx is None else tuple(u[idx] for u in d["upstream"])
    n = rays.n_rays
    dec = d["decoder"]
    params = dec.mlp_params.to(dtype).clone().requires_grad_(True)
    grids = [g.to(dtype).clone().requires_grad_(True) for g in d["grids"]]
    outs, g_enc = [[], [], []], []
    for lo in range(0, n, chunk):
        r = rays[lo:lo + chunk]
        for f in ("directions", "origins", "near", "far", "encoding"):
            setattr(r, f, getattr(r, f).to(dtype))
        r.encoding = r.encoding.clone().requires_grad_(True)
        dd = copy.copy(dec)
        dd.mlp_params = params
        out = O.lightplane_renderer_naive(r, grids, dd, **d["cfg"])
        u = [x[lo:lo + chunk].to(dtype) for x in up]
        ((out[0] * u[0]).sum() + (out[1] * u[1]).sum() + (out[2] * u[2]).sum()).backward()
        for k in range(3):
            outs[k].append(out[k].detach())
        g_enc.append(r.encoding.grad)
    return [torch.cat(o) for o in outs], params.grad, torch.cat(g_enc), [g.grad for g in grids]


def test_cfg2_full_batch_against_oracle():
    """All 65 536 rays of BASELINE configs[1]: the true scatter pattern of the headline launch (2 048 waves, one round of
    workgroups, 256^2 image on 64^2 planes) held to the oracle, every gradient family."""
    dev = _dev()
    d = cfg2_inputs()
    out, gp, ge, gg, _ = run_hip_renderer(d, dev, _lib.LP_KERNEL_AUTO)
    o_out, o_gp, o_ge, o_gg = oracle_chunked(d)   # the reference's arithmetic (fp32)
    for nm, a, b in (("ray_length", out[0], o_out[0]), ("neg_log_t", out[1], o_out[1]), ("feature", out[2], o_out[2])):
        _assert_close(f"cfg2 full: {nm}", a, b.numpy())
    # 65 536 x 128 samples x 128 hidden units = 1.07e9 pre-activations: ~1e-7 of them sit within fp32 round-off of zero, so a few
    # dozen rays carry a unit that any two fp32 evaluations decide differently.  The gradients are therefore PROVEN, not allowed
    # for: the kernel's own ReLU decisions forced onto the fp64 oracle (every forced unit a measured near tie), every entry at 1e-4.
    forced_oracle_check("cfg2 full", d, dev)
    # for the record: the unforced kernel and the fp32 oracle are flips apart (sparse: the relative L2 stays small)
    print("cfg2 full, unforced, relative L2 vs the fp32 oracle:",
          dict(grad_encoding=float((ge.cpu() - o_ge).norm() / o_ge.norm()), grad_mlp_params=float((gp.cpu() - o_gp).norm() / o_gp.norm()),
               grad_grid0=float((gg[0].cpu() - o_gg[0]).norm() / o_gg[0].norm())))


def test_baseline_cfg1_exact(golden_dir):
    """BASELINE configs[0] on the GPU: against the oracle and against the reference's own numbers."""
    dev = _dev()
    d = baseline_cfg1()
    z = np.load(os.path.join(golden_dir, "renderer__baseline_cfg1.npz"))
    for kernel, tag in ((_lib.LP_KERNEL_AUTO, "auto"), (_lib.LP_KERNEL_GENERIC, "generic")):
        out, gp, ge, gg, _ = run_hip_renderer(d, dev, kernel)
        o_out, o_gp, o_ge, o_gg = oracle_chunked(d)
        for nm, a, b in (("ray_length", out[0], o_out[0]), ("neg_log_t", out[1], o_out[1]), ("feature", out[2], o_out[2])):
            _assert_close(f"cfg1 {tag}: {nm}/oracle", a, b.numpy())
            _assert_close(f"cfg1 {tag}: {nm}/golden", a, z[nm])
        # gradients: the proof for both kernels (the kernel's own ReLU decisions forced onto the fp64 oracle, every entry at 1e-4)
        forced_oracle_check(f"cfg1 {tag}", d, dev, kernel=kernel)


@pytest.mark.parametrize("C,G,S", [(16, 64, 128), (32, 128, 64), (32, 128, 256)], ids=["c16_s128", "c32_s64", "cfg4_c32_s256"])
def test_1080p_backward_block(C, G, S):
    """A real 1920 x 1080 forward + backward launch; upstream gradient non-zero on a 24 x 40 block (not aligned to the 32-ray
    waves) only.  ``cfg4_c32_s256`` is BASELINE configs[3]'s per-GPU launch itself: triplane 128^2 x 32 ch at 256 samples."""
    dev = _dev()
    H, W = 1080, 1920
    gen = torch.Generator().manual_seed(7)
    sizes = grid_sizes_for((1, G, G, G, C), True)
    grids = random_grids(gen, sizes)
    dec = random_decoder(gen, 2, 2, 2, C, 32, 3, std=0.15)
    rays = pinhole_rays(H, W, enc_dim=32, gen=gen, azimuth_deg=35.0, elevation_deg=25.0)
    y0, x0, bh, bw = 517, 1003, 24, 40
    idx = (torch.arange(y0, y0 + bh)[:, None] * W + torch.arange(x0, x0 + bw)[None, :]).reshape(-1)
    n = H * W
    up = [torch.zeros(n), torch.zeros(n), torch.zeros(n, 3)]
    up[0][idx] = torch.randn(idx.numel(), generator=gen)
    up[1][idx] = torch.randn(idx.numel(), generator=gen)
    up[2][idx] = torch.randn(idx.numel(), 3, generator=gen)
    cfg = dict(num_samples=S, gain=1.0, num_samples_inf=0, mask_out_of_bounds_samples=False, contract_coords=False,
               inject_noise_sigma=0.0, inject_noise_seed=0)
    d = dict(rays=rays, grids=grids, color_grids=None, decoder=dec, scaffold=None, cfg=cfg, sizes=sizes, upstream=tuple(up))
    out, gp, ge, gg, _ = run_hip_renderer(d, dev, _lib.LP_KERNEL_AUTO)
    o_out = oracle_chunked(d, idx)[0]
    didx = idx.to(dev)
    for nm, a, b in (("ray_length", out[0], o_out[0]), ("neg_log_t", out[1], o_out[1]), ("feature", out[2], o_out[2])):
        _assert_close(f"1080p block: {nm}", a[didx], b.numpy())
    rest = torch.ones(n, dtype=torch.bool, device=dev)
    rest[didx] = False
    assert float(ge[rest].abs().max()) == 0.0, "rays without upstream gradient got an encoding gradient"
    # every gradient family of the WHOLE launch against the fp64 oracle of the block, the kernel's ReLU decisions forced (the proof)
    forced_oracle_check(f"1080p block C={C} S={S}", d, dev, idx)


# (cfg 2 full, the 1080p / cfg-4 blocks and cfg 1 are proven inside their own tests above: test_cfg2_full_batch_against_oracle,
# test_1080p_backward_block, test_baseline_cfg1_exact)
FLIP_PROOF_CASES = ["cfg2_segmented_64x64", "cfg2_segmented_noise_mask", "cfg2_64x64_inf8_contract",
                    # the layer-looped family (dump twins since 0.2.6): the golden cases of hidden 64 and of the 4/4/4 decoder, a
                    # two-grid decoder of hidden 64 and a segmented deep decoder on coherent images
                    "loop_triplane_h64_c32", "loop_triplane_deep444", "loop_two_grid_h64", "loop_segmented_deep444", "loop_example_112_h64"]


@pytest.mark.parametrize("case", FLIP_PROOF_CASES)
def test_flips_are_flips(case):
    """The ReLU-flip allowance of assert_grad_close, replaced by a proof on the launches bench.py times (round-4 review, next 2).
    The production backward's ReLU decisions are read back (lp_renderer_backward_relu_dump: the DUMP twin of the kernel that
    ran) and forced onto the fp64 oracle; EVERY entry of grad_grid / grad_encoding / grad_mlp_params and every output then
    meets 1e-4 outright.  cfg 2 full = the headline launch; the cfg-4 block = BASELINE configs[3]'s per-GPU launch; the
    segmented cases run the SEG instantiations (small batches; PLAIN and non-PLAIN), one case the non-PLAIN one-sweep kernel
    (beyond-far samples, contraction, opacity noise)."""
    dev = _dev()
    idx, fam = None, 1
    if case.startswith("loop_"):
        from tests.synth import RENDERER_CASES
        from tests.test_gpu_coherent import coherent_renderer_inputs
        fam = 3
        if case in ("loop_triplane_h64_c32", "loop_triplane_deep444"):
            d = next(c for c in RENDERER_CASES if c.name == case[len("loop_"):]).build()
        elif case == "loop_two_grid_h64":
            d = coherent_renderer_inputs("two_grid_triplane_c16", "48x80_az30_el45", seed=3, hidden=64)
        elif case == "loop_example_112_h64":
            d = coherent_renderer_inputs("triplane24_c32_t1o1c2", "48x80_az30_el45", seed=3, hidden=64)
        else:
            d = coherent_renderer_inputs("triplane24_c16_deep444", "64x64_axis", num_samples=72, seed=11)
            assert lp.backward_segments(d["rays"], d["grids"], d["decoder"], **d["cfg"]) > 1, "this case must run the segmented kernels"
    elif case == "cfg2_64x64_inf8_contract":  # the non-PLAIN kernel, one sweep per ray (beyond-far samples are never segmented)
        d = cfg2_inputs(height=64, width=64)
        d["cfg"] = dict(d["cfg"], num_samples_inf=8, contract_coords=True, inject_noise_sigma=0.3, inject_noise_seed=5)
    elif case.startswith("cfg2_segmented"):
        d = cfg2_inputs(height=64, width=64)
        if case.endswith("noise_mask"):  # the non-PLAIN SEG instantiation
            d["cfg"] = dict(d["cfg"], inject_noise_sigma=0.3, inject_noise_seed=11, mask_out_of_bounds_samples=True)
        assert lp.backward_segments(d["rays"], d["grids"], d["decoder"], num_samples=d["cfg"]["num_samples"],
                                    num_samples_inf=d["cfg"].get("num_samples_inf", 0)) > 1, "this case must run the segmented kernels"
    assert lp.kernel_family(d["rays"], d["grids"], d["decoder"], color_grid=d["color_grids"]) == fam
    # (the opacity noise is a hash of the GLOBAL ray index and the ray count: a noisy case goes through the oracle in one chunk)
    forced_oracle_check(case, d, dev, idx, chunk=2048 if d["cfg"]["inject_noise_sigma"] == 0 else d["rays"].n_rays)


def test_cfg2_fp32_arithmetic_agrees_with_default():
    """LpRendererArgs.arithmetic = LP_ARITH_FP32 on the headline launch (all 65 536 rays): the reference's arithmetic -- three limbs in
    the dX chains, fp32 weight-gradient products -- selected per call, no rebuild.  Forward and recompute are the same instruction
    sequence in both modes, so the outputs are bit-identical and the ReLU decisions agree: the two backwards differ by the limb
    truncation of the default mode and the order of the fp32 atomics only, far inside 1e-4."""
    dev = _dev()
    d = cfg2_inputs()
    assert lp.kernel_family(d["rays"], d["grids"], d["decoder"], arithmetic=_lib.LP_ARITH_FP32) == 1
    out0, gp0, ge0, gg0, _ = run_hip_renderer(d, dev, _lib.LP_KERNEL_AUTO)
    out1, gp1, ge1, gg1, _ = run_hip_renderer(d, dev, _lib.LP_KERNEL_AUTO, arithmetic=_lib.LP_ARITH_FP32)
    for a, b in zip(out0, out1):
        assert torch.equal(a, b)
    worst = {}
    for nm, a, b in [("grad_mlp_params", gp0, gp1), ("grad_encoding", ge0, ge1)] + [(f"grad_grid{i}", a, b) for i, (a, b) in enumerate(zip(gg0, gg1))]:
        worst[nm] = float((a - b).abs().max() / b.abs().max())
    print("cfg2 full: default (two-limb dX / dW) vs LP_ARITH_FP32 backward, max |diff| / max |ref|:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert max(worst.values()) <= 5e-5, worst


def test_relu_dump_refuses_kernels_without_a_twin():
    """Every kernel family has dump twins; the LP_ARITH_FP32 instantiations do not and must refuse loudly (never a silent production
    launch).  The shape-generic twin writes ceil(widest site / 32) words per site."""
    from lightplane_amd.renderer import relu_dump_recorder, relu_dump_words
    from tests.synth import RENDERER_CASES
    dev = _dev()
    d = next(c for c in RENDERER_CASES if c.name == "triplane_deep444").build()
    with relu_dump_recorder():
        with pytest.raises(_lib.LightplaneHipError, match="relu dump"):
            run_hip_renderer(d, dev, _lib.LP_KERNEL_AUTO, arithmetic=_lib.LP_ARITH_FP32)
    n_sites = len(relu_site_widths(d))
    assert relu_dump_words(d["rays"], d["grids"], d["decoder"], kernel=_lib.LP_KERNEL_GENERIC) == n_sites * 1 + 1   # hidden 32
    forced_oracle_check("deep444 generic", d, dev, kernel=_lib.LP_KERNEL_GENERIC)


INDEX_CASES = {
    # name: (grid base, triplane, image H, W, azimuth, elevation, samples)
    "triplane20_c16": ((1, 20, 24, 28, 16), True, 48, 80, 30.0, 45.0, 24),
    "triplane16_c32": ((1, 16, 16, 16, 32), True, 64, 64, 0.0, 0.0, 20),
    "voxel14_c16": ((1, 14, 12, 18, 16), False, 48, 80, 30.0, 45.0, 24),
    "voxel12_c32_b2": ((2, 12, 12, 12, 32), False, 40, 48, 60.0, -20.0, 16),
}


@pytest.mark.parametrize("layers", [(2, 2, 2), (4, 4, 4)], ids=["tuned222", "looped444"])
@pytest.mark.parametrize("name", list(INDEX_CASES), ids=list(INDEX_CASES))
def test_hot_kernel_touched_rows_equal_oracle(name, layers):
    """Integer indexing of the PRODUCTION kernels: the rows of grad_grid the MFMA backward writes are exactly the rows the
    oracle's corner indices name (the camera sits close enough that rays leave the volume: border cells, partly valid
    corners and rays that miss a plane altogether all occur)."""
    dev = _dev()
    base, tri, H, W, az, el, S = INDEX_CASES[name]
    gen = torch.Generator().manual_seed(3)
    sizes = grid_sizes_for(base, tri)
    grids = random_grids(gen, sizes)
    C = base[-1]
    dec = random_decoder(gen, *layers, C, 32, 3, std=0.2 if layers == (2, 2, 2) else 0.25)
    parts = [pinhole_rays(H, W, cam_dist=2.2, enc_dim=32, gen=gen, grid_idx=b, azimuth_deg=az + 50.0 * b, elevation_deg=el)
             for b in range(base[0])]
    from tests.synth import cat_rays
    rays = parts[0] if len(parts) == 1 else cat_rays(parts)
    n = rays.n_rays
    up = (torch.randn(n, generator=gen), torch.randn(n, generator=gen) + 3.0, torch.randn(n, 3, generator=gen))
    cfg = dict(num_samples=S, gain=1.0, num_samples_inf=0, mask_out_of_bounds_samples=False, contract_coords=False,
               inject_noise_sigma=0.0, inject_noise_seed=0)
    d = dict(rays=rays, grids=grids, color_grids=None, decoder=dec, scaffold=None, cfg=cfg, sizes=sizes, upstream=up)
    fam = lp.kernel_family(rays, grids, dec)
    assert fam != 0, "this test is about the MFMA kernels"
    if layers == (4, 4, 4):  # the layer-looped family has its OWN gather / scatter specialisations (lp_renderer_loop.hip)
        assert fam == 3, fam
    _, _, _, gg, _ = run_hip_renderer(d, dev, _lib.LP_KERNEL_AUTO)
    rows = O.renderer_corner_indices(rays, sizes, S, 0, False)  # per grid: [N, S, K] rows relative to the grid (-1: outside)
    _, _, _, o_gg = oracle_chunked(d)
    for g, (got, want_rows, o_g) in enumerate(zip(gg, rows, o_gg)):
        touched = (got.reshape(-1, C) != 0).any(dim=1).cpu()
        named = torch.zeros_like(touched)
        r = want_rows.reshape(-1)
        named[r[r >= 0]] = True
        spurious = int((touched & ~named).sum())
        assert spurious == 0, f"{name} grid {g}: {spurious} rows written that no corner of the oracle names"
        o_touched = (o_g.reshape(-1, C) != 0).any(dim=1)
        assert torch.equal(touched, o_touched), (f"{name} grid {g}: touched-row sets differ in "
                                                  f"{int((touched != o_touched).sum())} of {touched.numel()} rows")
        assert int(touched.sum()) > 0.3 * touched.numel() and int((~named).sum()) >= 0


@pytest.mark.parametrize("which", ["ref_fixture_std0.01", "grid_1e3_weights_1e-3", "mixed_magnitudes_deep"])
def test_bf16x3_operand_dynamic_range(which):
    """The decoder products run as bf16x3 (three bf16 limbs per fp32 operand) -- exact splits, so the accuracy must not
    depend on operand magnitudes.  The parity cases draw weights from N(0, 0.15-0.3) and grids from N(0, 1); here: the
    reference fixture's own N(0, 0.01) parameters (tests/utils.py:349), grid features of ~1e3 against weights of ~1e-3, and a
    deep decoder (layer-looped family) whose layers alternate between scales 8 and 1/8 with per-channel grid scales over six
    decades -- all held to the fp32 oracle at the 1e-4 bar."""
    dev = _dev()
    gen = torch.Generator().manual_seed(11)
    C, H = 16, 32
    layers = (4, 3, 4) if which == "mixed_magnitudes_deep" else (2, 2, 2)
    sizes = grid_sizes_for((1, 12, 14, 10, C), True)
    grids = random_grids(gen, sizes)
    std = 0.01 if which == "ref_fixture_std0.01" else 0.2
    dec = random_decoder(gen, *layers, C, H, 3, std=std)
    if which == "grid_1e3_weights_1e-3":
        grids = [g * 1e3 for g in grids]
        p = dec.mlp_params.clone()
        p[: C * H] *= 1e-3  # first trunk layer's weights
        dec.mlp_params = p
    if which == "mixed_magnitudes_deep":
        scale = 10.0 ** torch.linspace(-3, 3, C)
        grids = [g * scale for g in grids]
        p = dec.mlp_params.clone()
        p[: C * H] = p[: C * H].reshape(C, H) .div(scale[:, None]).reshape(-1)  # undo the channel scales in the first layer
        off = C * H
        for l in range(3):  # the three hidden trunk layers: x8, /8, x8 (the next layer's weights compensate)
            f = 8.0 if l % 2 == 0 else 0.125
            p[off: off + H * H] *= f
            off += H * H
        dec.mlp_params = p
    rays = pinhole_rays(40, 48, cam_dist=2.4, enc_dim=H, gen=gen, azimuth_deg=25.0, elevation_deg=15.0)
    n = rays.n_rays
    up = (torch.randn(n, generator=gen), torch.randn(n, generator=gen), torch.randn(n, 3, generator=gen))
    cfg = dict(num_samples=24, gain=1.0 if which != "ref_fixture_std0.01" else 3.0, num_samples_inf=0, mask_out_of_bounds_samples=False,
               contract_coords=False, inject_noise_sigma=0.0, inject_noise_seed=0)
    d = dict(rays=rays, grids=grids, color_grids=None, decoder=dec, scaffold=None, cfg=cfg, sizes=sizes, upstream=up)
    assert lp.kernel_family(rays, grids, dec) in (1, 3)
    out = run_hip_renderer(d, dev, _lib.LP_KERNEL_AUTO)[0]
    o_out = oracle_chunked(d)[0]
    for nm, a, b in (("ray_length", out[0], o_out[0]), ("neg_log_t", out[1], o_out[1]), ("feature", out[2], o_out[2])):
        _assert_close(f"{which}: {nm}", a, b.numpy())
    forced_oracle_check(which, d, dev)  # every gradient entry at 1e-4 against fp64 with the kernel's ReLU decisions


# --------------------------------------------------------------------------------------------------------------
# BASELINE configs[2] (cfg 3) at FULL size, and index parity of the Splatter walks
# --------------------------------------------------------------------------------------------------------------


def splatter_oracle_chunked(rays, shape, cfg, upstream, chunk=1024):
    """The Splatter oracle over all rays in ray chunks: un-normalised feature / weight sums accumulated with the oracle's own
    corner arithmetic (oracle._corner_setup with the Splatter's un-normalisation, oracle.ray_depths), normalised once at the
    end like oracle._splatter_impl; grad_encoding = the adjoint gather of upstream / clamp(weight) with the same corners.
    (oracle._splatter_impl itself materialises [N, S, C] tensors and out-of-place index_adds of the whole grid: 65 536 rays x
    256 samples do not fit; this is the same arithmetic in chunks, fp32.)"""
    B, D, H, W, C = shape
    n = rays.n_rays
    old_threads = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    try:
        fgrid = torch.zeros(B * D * H * W, C)
        wgrid = torch.zeros(B * D * H * W)

        def corners(lo):
            r = rays[lo:lo + chunk]
            depths = O.ray_depths(r.near, r.far, cfg["num_samples"], cfg.get("num_samples_inf", 0), 1e-5)
            pts = depths[..., None] * r.directions[:, None] + r.origins[:, None]
            assert not cfg.get("contract_coords", False)
            mask = O.in_bounds(pts).float() if cfg.get("mask_out_of_bounds_samples", False) else torch.ones(pts.shape[:-1])
            gi = r.grid_idx.long()
            for idx, w, valid in O._corner_setup(pts, shape, O._unnormalize_splatter):
                yield r, (gi[:, None] * (D * H * W) + idx), w * valid.float() * mask

        with torch.no_grad():
            for lo in range(0, n, chunk):
                for r, rows, w in corners(lo):
                    wgrid.index_add_(0, rows.reshape(-1), w.reshape(-1))
                    val = r.encoding[:, None, :] * w[..., None]
                    fgrid.index_add_(0, rows.reshape(-1), val.reshape(-1, C))
            out = fgrid / wgrid.clamp(min=1e-5)[:, None]
            g = upstream.reshape(-1, C) / wgrid.clamp(min=1e-5)[:, None]
            g_enc = torch.zeros(n, C)
            for lo in range(0, n, chunk):
                for r, rows, w in corners(lo):
                    g_enc[lo:lo + chunk] += (g[rows.reshape(-1)].reshape(rows.shape + (C,)) * w[..., None]).sum(dim=1)
        return out.reshape(B, D, H, W, C), g_enc, wgrid.reshape(B, D, H, W)
    finally:
        torch.set_num_threads(old_threads)


def test_splatter_chunked_oracle_equals_oracle_cpu_part():
    """(runs on the GPU box, CPU work only) the chunked restatement above == oracle.lightplane_splatter_naive + autograd on a
    case small enough for both."""
    gen = torch.Generator().manual_seed(5)
    rays = pinhole_rays(24, 40, cam_dist=2.3, azimuth_deg=20.0, elevation_deg=35.0)
    rays.encoding = torch.rand(rays.n_rays, 32, generator=gen).requires_grad_(True)
    shape = [1, 12, 14, 10, 32]
    cfg = dict(num_samples=20, num_samples_inf=0, mask_out_of_bounds_samples=True, contract_coords=False)
    up = torch.randn(*shape, generator=gen)
    (want,) = O.lightplane_splatter_naive(rays, [shape], **cfg)
    (want * up).sum().backward()
    with torch.no_grad():
        got, g_enc, _ = splatter_oracle_chunked(rays, shape, cfg, up, chunk=100)
    _assert_close("chunked oracle: out", got, want.detach().numpy(), tol=2e-6)
    _assert_close("chunked oracle: grad_encoding", g_enc, rays.encoding.grad.numpy(), tol=2e-6)


def test_cfg3_full_batch_against_oracle():
    """BASELINE configs[2] at full size -- 65 536 rays of the 256 x 256 camera x 32 ch, 256 samples, into the 128^3 x 32 voxel
    grid (the launch bench.py's `splatter_cfg3` times): the whole output grid and grad_encoding against the chunked CPU oracle."""
    from bench import SplatterWorkload
    dev = _dev()
    wl = SplatterWorkload(0, dev, None)
    rays_c, shape = wl.rays_c, wl.sizes[0]
    cfg = dict(num_samples=wl.S, num_samples_inf=0, mask_out_of_bounds_samples=False, contract_coords=False)
    up = wl.up.cpu().reshape(*shape)
    rays = rays_c.to(dev)
    rays.encoding = rays.encoding.clone().requires_grad_(True)
    (out,) = lp.lightplane_splatter(rays, [shape], **cfg)
    (out * up.to(dev)).sum().backward()
    want, want_ge, wgrid = splatter_oracle_chunked(rays_c, shape, cfg, up)
    _assert_close("cfg3 full: out", out, want.numpy())
    _assert_close("cfg3 full: grad_encoding", rays.encoding.grad, want_ge.numpy())
    num = (rays.encoding.grad.double().cpu() - want_ge.double()).norm().item()
    assert num / want_ge.double().norm().item() <= 1e-4, "cfg3 full: grad_encoding relative L2"
    num = (out.double().cpu() - want.double()).norm().item()
    assert num / want.double().norm().item() <= 1e-4, "cfg3 full: out relative L2"
    # integer indexing of the walk at full scale: a cell received weight on the GPU iff it did in the oracle
    assert torch.equal((out != 0).any(dim=-1).cpu(), wgrid > 0), "cfg3 full: touched cells differ from the oracle's"
    assert int((wgrid > 0).sum()) > 100000


def _footprint_box(rays, shape, S):
    """Bounding box ((z0, z1), (y0, y1), (x0, x1)) of the cells the Renderer's samples of ``rays`` touch with non-zero weight
    (oracle.renderer_corner_indices' corners, the reference's fp32 geometry), and the flat indices of those cells."""
    _, D, H, W, _ = shape
    depths = O.ray_depths(rays.near, rays.far, S, 0, 1e-5)
    pts = depths[..., None] * rays.directions[:, None] + rays.origins[:, None]
    cells = torch.cat([idx[valid & (w != 0)] for idx, w, valid in O._corner_setup(pts, shape, O._unnormalize_renderer)]).unique()
    z, y, x = cells // (H * W), (cells // W) % H, cells % W
    box = tuple((int(a.min()), int(a.max()) + 1) for a in (z, y, x))
    return box, cells


def _oracle_render_forward(rays, grid64, decoder, cfg, chunk=512):
    """fp64 oracle forward (fp32 geometry) of ``rays`` on the fp64 grid ``grid64``, in chunks; no gradients."""
    dec = copy.copy(decoder)
    dec.mlp_params = decoder.mlp_params.to(F64)
    outs = [[], [], []]
    with torch.no_grad(), O.geometry_dtype(torch.float32):
        for lo in range(0, rays.n_rays, chunk):
            r = rays[lo:lo + chunk]
            r.encoding = r.encoding.to(F64)
            for k, o in enumerate(O.lightplane_renderer_naive(r, [grid64], dec, **cfg)):
                outs[k].append(o)
    return [torch.cat(o) for o in outs]


def test_cfg5_full_chain_against_oracle(monkeypatch):
    """BASELINE configs[4] at the size bench.py's `cfg5` times, one chained step through JointWorkload.forward itself: 13 views x 512^2
    rays splatted into the 256^3 x 32 voxel grid (2.15 GB: the ray-block-major forward walk, 26 624 ray blocks; the backward with one
    segment, grad_encoding a plain store; 4-row patches of 512-ray rows over 13 views), normalised over 2^29 entries, then 135 x 1920 rays
    of a 1080p camera rendered from it at S = 256 (the 3-waves-per-SIMD forward), the end-to-end backward.  The upstream gradient is
    non-zero on a 24 x 40 render block (not aligned to the 32-ray waves) only.  Held to fp64 oracles:

    A. the kernel's weight grid (the first tensor LightplaneSplatterFunction saves) against the in-place fp64 weight pass over all
       16.7 M cells at 1e-4, the cells with weight > 0 exactly the oracle's; the splat finite and in [0, 1) everywhere;
    B. the splat's values against oracle.splatter_box_oracle on four boxes (the render block's footprint, the grid's low and high index
       corners, an interior box) at 1e-4;
    C. the Renderer on the grid it was given: forced_oracle_check on the block (every output and gradient entry, the whole 2.15 GB grid
       gradient included, at 1e-4); the chain's render outputs bit-identical to that launch's, its retained grid gradient within the
       2e-5 of fp32 atomic order; every 63rd ray's outputs (all 135 rows, every lane) against the fp64 oracle forward at 1e-4;
    D. the chain into the splat encodings: every candidate ray of the box oracle's prefilter (upstream = the forced oracle's grid
       gradient, the weights of A) at 1e-4, every other of the 3 407 872 rays exactly 0;
    E. end to end: the block's render outputs against box-oracle splat -> fp64 oracle render (the grid zero outside the footprint box).

    The block and the boxes were chosen with the oracle alone; the test asserts that they are not vacuous.  Run time on one MI355X with
    the oracle on 16 host threads (the printed `cfg5 full chain: time` line): 52-54 s -- the chained step 2.6 s, the forced proof of the
    render block 8.3 s (its two GPU launches and the fp64 oracle), the other host oracles 42 s (the weight pass over 872 M samples, the
    box oracles, the oracle renders).  In the same run test_cfg3_full_batch_against_oracle took under 5 s, the whole GPU suite 4.4 min."""
    import time

    import bench
    from tests.test_gpu_parity import forced_oracle_check

    for k in ("CFG5_VIEWS", "CFG5_IMG", "CFG5_GRID", "CFG5_ROWS", "CFG5_S", "LP_BENCH_NO_ROW_HINT"):
        monkeypatch.delenv(k, raising=False)
    dev = _dev()
    t_gpu, t_cpu = 0.0, 0.0
    t = time.time()
    wl = bench.JointWorkload(0, 1, dev, None, _lib.LP_KERNEL_AUTO)
    assert (wl.V, wl.img, wl.G, wl.rows, wl.S, wl.C) == (13, 512, 256, 135, 256, 32)
    shape = wl.sizes[0]
    assert shape == [1, 256, 256, 256, 32] and wl.splat_rays.n_rays == 13 * 512 * 512 and wl.cam.n_rays == 135 * 1920
    n_cells = 256 ** 3
    assert n_cells * 32 * 4 > 1e9, "the grid has to select the ray-block-major forward walk (splat_forward_group: > 1 GB)"
    S = wl.S

    # the render block (rows 100..123 of the 135, columns 941..980: 941 = 29 * 32 + 13) and its upstream gradient
    Wimg, y0, x0, bh, bw = 1920, 100, 941, 24, 40
    idx = (torch.arange(y0, y0 + bh)[:, None] * Wimg + torch.arange(x0, x0 + bw)[None, :]).reshape(-1)
    n = wl.cam.n_rays
    gen = torch.Generator().manual_seed(55)
    up = [torch.zeros(n), torch.zeros(n), torch.zeros(n, 3)]
    up[0][idx] = torch.randn(idx.numel(), generator=gen)
    up[1][idx] = torch.randn(idx.numel(), generator=gen)
    up[2][idx] = torch.randn(idx.numel(), 3, generator=gen)

    # one chained step, recording the splat the Renderer consumed and the weight grid its launch produced
    captured = {}
    splatter = bench.lp.lightplane_splatter

    def recording_splatter(*args, **kw):
        saved = []

        def pack(x):
            saved.append(x)
            return x

        with torch.autograd.graph.saved_tensors_hooks(pack, lambda x: x):
            grid = splatter(*args, **kw)
        grid.retain_grad()
        captured.update(grid=grid, weight=saved[0], kw=kw)
        return grid

    monkeypatch.setattr(bench.lp, "lightplane_splatter", recording_splatter)
    wl.zero_grads()
    out = wl.forward(replicated=False)
    torch.autograd.backward(list(out[:3]), [u.to(dev) for u in up])
    torch.cuda.synchronize(dev)
    monkeypatch.setattr(bench.lp, "lightplane_splatter", splatter)
    grid, wk = captured["grid"].detach(), captured["weight"]
    assert captured["kw"].get("rays_per_row") == 512, "the chain has to run with bench.py's row-length hint"
    assert wk.shape == (n_cells,) and wk.dtype == torch.float32 and grid.shape == (n_cells, 32)
    g_chain = captured["grid"].grad
    ge_chain = wl.splat_rays.encoding.grad
    out = [o.detach() for o in out[:3]]
    t_gpu += time.time() - t

    old_threads = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    try:
        # A. the weight grid, whole grid
        t = time.time()
        rays_c = wl.splat_rays.to("cpu")
        rays_c.encoding = rays_c.encoding.detach()
        cfg_s = dict(num_samples=S, num_samples_inf=0, mask_out_of_bounds_samples=False, contract_coords=False)
        (w_or,) = O.splatter_weight_grids(rays_c, [shape], S, sum_dtype=F64)
        w_or = w_or[:, 0]
        t_cpu += time.time() - t
        wk_c = wk.cpu()
        _assert_close("cfg5 full: weight grid", wk_c, w_or.numpy())
        assert torch.equal(wk_c > 0, w_or > 0), f"cfg5 full: cells with weight differ in {int(((wk_c > 0) != (w_or > 0)).sum())} cells"
        assert bool(torch.isfinite(grid).all()) and float(grid.min()) >= 0.0 and float(grid.max()) < 1.0
        del wk_c

        # B. the splat's values on four boxes
        t = time.time()
        cam_c = wl.cam.to("cpu")
        fbox, fcells = _footprint_box(cam_c[idx], shape, S)
        boxes = {"footprint": fbox, "low_corner": ((0, 24), (0, 24), (0, 24)), "high_corner": ((232, 256), (232, 256), (232, 256)),
                 "interior": ((116, 140), (116, 140), (116, 140))}
        box_res = {}
        for nm, box in boxes.items():
            res = O.splatter_box_oracle(rays_c, shape, box, cfg_s)
            box_res[nm] = res
            assert int((res.weight_sums > 0).sum()) >= 1000, f"value box {nm} {box}: too few cells with weight"
            (z0, z1), (yb0, yb1), (xb0, xb1) = box
            got = grid.reshape(256, 256, 256, 32)[z0:z1, yb0:yb1, xb0:xb1]
            _assert_close(f"cfg5 full: splat values, {nm} box {box}", got, (res.feature_sums / res.weight_sums.clamp(min=1e-5)[..., None]).numpy())
        t_cpu += time.time() - t

        # C. the Renderer on the grid it was given: the forced fp64 proof of the whole launch on the block
        t = time.time()
        cam_c.encoding = cam_c.encoding.detach()
        grid_c = grid.cpu().reshape(shape)
        cfg_r = dict(num_samples=S, gain=1.0, num_samples_inf=0, mask_out_of_bounds_samples=False, contract_coords=False,
                     inject_noise_sigma=0.0, inject_noise_seed=0)
        d = dict(rays=cam_c, grids=[grid_c], color_grids=None, decoder=wl.dec_c, scaffold=None, cfg=cfg_r, sizes=[shape], upstream=tuple(up))
        _, prod, forced = forced_oracle_check("cfg5 full chain: render block", d, dev, idx, return_results=True)
        t_proof = time.time() - t
        for k in range(3):
            assert torch.equal(out[k], prod[0][k]), f"cfg5 full: chained render output {k} differs from the proof launch's"
        err = float((g_chain.reshape(-1) - prod[3][0].reshape(-1)).abs().max() / prod[3][0].abs().max())
        assert err <= 2e-5, f"cfg5 full: retained grid gradient vs the proof launch's {err:.3e}"
        f_gg = forced[3][0].reshape(n_cells, 32)
        del prod
        t = time.time()
        sidx = torch.arange(0, n, 63)
        assert sidx.numel() >= 4096 and (sidx // Wimg).unique().numel() == 135 and (sidx % 32).unique().numel() == 32
        grid64 = grid_c.to(F64)
        o_sub = _oracle_render_forward(cam_c[sidx], grid64, wl.dec_c, cfg_r)
        for k, nm in enumerate(("ray_length", "neg_log_t", "feature")):
            _assert_close(f"cfg5 full: every 63rd ray, {nm}", out[k][sidx.to(dev)], o_sub[k].numpy())

        # D. the chain into the splat encodings
        nz = (f_gg != 0).any(dim=-1)
        assert int(nz[fcells].sum()) >= 1000 and int(nz.sum()) == int(nz[fcells].sum())
        res = O.splatter_box_oracle(rays_c, shape, fbox, cfg_s, upstream=f_gg, weights=w_or)
        cand = res.candidates
        assert int((res.grad_encoding != 0).any(dim=-1).sum()) >= 1000
        dc = cand.to(dev)
        _assert_close("cfg5 full: grad_encoding of the prefilter's candidate rays", ge_chain[dc], res.grad_encoding[cand].numpy())
        assert float(ge_chain[~dc].abs().max()) == 0.0, "cfg5 full: a ray that cannot reach the footprint box got an encoding gradient"

        # E. end to end: box-oracle splat -> fp64 oracle render, on a grid zero outside the footprint box
        r = box_res["footprint"]
        (z0, z1), (yb0, yb1), (xb0, xb1) = fbox
        grid64.zero_()
        grid64[0, z0:z1, yb0:yb1, xb0:xb1] = r.feature_sums / r.weight_sums.clamp(min=1e-5)[..., None]
        o_blk = _oracle_render_forward(cam_c[idx], grid64, wl.dec_c, cfg_r)
        for k, nm in enumerate(("ray_length", "neg_log_t", "feature")):
            _assert_close(f"cfg5 full: end to end, block {nm}", out[k][idx.to(dev)], o_blk[k].numpy())
        t_cpu += time.time() - t
    finally:
        torch.set_num_threads(old_threads)
    print(f"cfg5 full chain: time: chained step {t_gpu:.1f} s, forced proof of the render block (GPU launches + fp64 oracle) {t_proof:.1f} s, "
          f"other host oracles {t_cpu:.1f} s; footprint box {fbox} ({fcells.numel()} cells), {int(cand.sum())} candidate splat rays, "
          f"{res.n_samples} samples evaluated")


SPLAT_INDEX_CASES = {
    # name: (out_base, triplane, H, W, azimuth, elevation, samples, mask_oob)
    "voxel14_c16": ((1, 14, 12, 18, 16), False, 48, 80, 30.0, 45.0, 24, False),
    "voxel12_c32_b2_mask": ((2, 12, 12, 12, 32), False, 40, 48, 60.0, -20.0, 16, True),
    "voxel10_c64": ((1, 10, 12, 14, 64), False, 40, 48, 15.0, 20.0, 20, False),
    "triplane20_c16": ((1, 20, 24, 28, 16), True, 48, 80, 30.0, 45.0, 24, False),
    "triplane16_c32_mask": ((1, 16, 16, 16, 32), True, 64, 64, 0.0, 0.0, 20, True),
    "triplane12_c64": ((1, 12, 10, 14, 64), True, 40, 48, 40.0, 10.0, 18, False),
}


@pytest.mark.parametrize("name", list(SPLAT_INDEX_CASES), ids=list(SPLAT_INDEX_CASES))
def test_splatter_walk_touched_cells_equal_oracle(name):
    """Integer indexing of the PRODUCTION Splatter walks (lp_splat_walk.h: the voxel column walk with carried columns, the
    per-slot plane walk; C = 16 / 32 / 64) -- which use the Splatter oracle's own un-normalisation `(x + 1) / 2 * W - 0.5`, not
    the Renderer's: with strictly positive features a cell of the output is non-zero iff it received weight, so the non-zero
    cells of the GPU output must be EXACTLY the cells the oracle's weight grid marks.  The camera sits close enough that rays
    leave the volume (border cells, partly valid corners, rays that miss altogether)."""
    from tests.synth import cat_rays
    dev = _dev()
    base, tri, H, W, az, el, S, mask = SPLAT_INDEX_CASES[name]
    gen = torch.Generator().manual_seed(4)
    C = base[-1]
    sizes = grid_sizes_for(base, tri)
    parts = [pinhole_rays(H, W, cam_dist=2.2, grid_idx=b, azimuth_deg=az + 50.0 * b, elevation_deg=el) for b in range(base[0])]
    rays = parts[0] if len(parts) == 1 else cat_rays(parts)
    rays.encoding = 0.5 + 0.5 * torch.rand(rays.n_rays, C, generator=gen)
    cfg = dict(num_samples=S, num_samples_inf=0, mask_out_of_bounds_samples=mask, contract_coords=False)
    out = lp.lightplane_splatter(rays.to(dev), sizes, **cfg)
    for g, (got, shape) in enumerate(zip(out, sizes)):
        _, _, wgrid = splatter_oracle_chunked(rays, shape, cfg, torch.zeros(*shape))
        touched = (got != 0).any(dim=-1).cpu()
        assert torch.equal(touched, wgrid > 0), (f"{name} grid {g}: touched cells differ in {int((touched != (wgrid > 0)).sum())} of "
                                                 f"{touched.numel()} cells")
        assert 0.2 * touched.numel() < int(touched.sum()) and bool((got >= 0).all())


# --------------------------------------------------------------------------------------------------------------
# transposed march of the tuned backward (LpRendererArgs.march_order = LP_MARCH_SAMPLES_PER_WAVE): batches of unrelated rays
# --------------------------------------------------------------------------------------------------------------

def _random_ray_case(n_rays, C, S, triplane=True, B=3, G=32, color_chn=3, seed=0, std=0.2, mask=False, rich=False):
    """The reference benchmark's kind of input (tests/renderer_speed_benchmark.py:228-246, tests/utils.py:230-268): random rays over
    B batch entries of a coarse grid, 2/2/2 x 32 decoder."""
    from tests.synth import random_rays
    gen = torch.Generator().manual_seed(seed)
    sizes = grid_sizes_for((B, G, G, G, C), triplane)
    grids = random_grids(gen, sizes)
    dec = random_decoder(gen, 2, 2, 2, C, 32, color_chn, std=std)
    rays = random_rays(gen, n_rays, B, 32)
    up = (torch.randn(n_rays, generator=gen), torch.randn(n_rays, generator=gen), torch.randn(n_rays, color_chn, generator=gen))
    cfg = dict(num_samples=S, gain=1.0, num_samples_inf=0, mask_out_of_bounds_samples=mask, contract_coords=False, inject_noise_sigma=0.0,
               inject_noise_seed=0)
    scaffold = None
    if rich:  # the non-PLAIN instantiations: opacity noise, contraction, an occupancy scaffold
        cfg.update(contract_coords=True, inject_noise_sigma=0.4, inject_noise_seed=17)
        scaffold = (torch.rand(B, 6, 5, 7, generator=gen) > 0.3).float()
    return dict(rays=rays, grids=grids, color_grids=None, decoder=dec, scaffold=scaffold, cfg=cfg, sizes=sizes, upstream=up)


@pytest.mark.parametrize("n_rays,C,S,tri,cc,mask,rich", [(4096, 32, 256, True, 3, False, False), (3000, 16, 100, True, 3, True, False),
                                                         (2500, 32, 40, False, 4, False, False), (140000, 16, 33, True, 3, False, False),
                                                         (777, 16, 32, False, 1, True, False), (3100, 16, 70, True, 3, False, True),
                                                         (2100, 32, 64, False, 4, False, True)],
                         ids=["refbench_like_c32_s256", "c16_s100_mask", "voxel_c32_rgba_s40", "140k_rays_32_per_wave_s33", "voxel_c16_tail_wave_s32",
                              "c16_s70_noise_contract_scaffold", "voxel_c32_rgba_s64_noise_contract_scaffold"])
def test_transposed_march_on_random_rays(n_rays, C, S, tri, cc, mask, rich):
    """march_order="samples" (one ray x 32 consecutive samples per wavefront: the run merge of the gradient scatter works along the
    ray) against march_order="rays" of the same kernels' arithmetic -- same forward, same recompute, so the same ReLU decisions:
    every gradient within 2e-5 -- and PROVEN against the fp64 oracle (its DUMP twin's decisions forced, every entry at 1e-4).
    Ragged sample counts (a last block of 1 .. 8 samples), a last wave with fewer rays, 1 .. 32 rays per wave (small batches are
    dealt over more workgroups), voxel and triplane scatter walks, three / four colour channels, masked samples."""
    dev = _dev()
    d = _random_ray_case(n_rays, C, S, triplane=tri, color_chn=cc, mask=mask, seed=n_rays % 97, rich=rich)
    assert lp.kernel_family(d["rays"], d["grids"], d["decoder"]) == 1
    ref = run_hip_renderer(d, dev, _lib.LP_KERNEL_AUTO, march_order="rays")
    got = run_hip_renderer(d, dev, _lib.LP_KERNEL_AUTO, march_order="samples")
    import ctypes
    last = _lib.lib().lp_debug_last_renderer_backward
    last.restype = ctypes.c_char_p
    assert b"transposed march" in last(), f"march_order='samples' did not launch the transposed-march backward: {last()}"  # never a silent fall-back
    for nm, a, b in zip(("ray_length", "neg_log_t", "feature"), got[0], ref[0]):  # the transposed forward: same samples, a scan instead of a loop
        _assert_close(f"transposed forward vs rays-per-wavefront forward: {nm}", a, b.detach().cpu().numpy(), tol=3e-6)
    scaff = dict(scaffold=d["scaffold"]) if rich else {}
    assert lp.backward_segments(d["rays"], d["grids"], d["decoder"], **d["cfg"], **scaff) == (1 if n_rays > 32768 else -(-S // _lib.LP_SEG_LEN))
    assert lp.backward_segments(d["rays"], d["grids"], d["decoder"], march_order="samples", **d["cfg"], **scaff) == 1  # dealt by rays per wave instead
    flat = lambda r: [("grad_mlp_params", r[1]), ("grad_encoding", r[2])] + [(f"grad_grid{i}", g) for i, g in enumerate(r[3])]  # noqa: E731
    for (nm, a), (_, b) in zip(flat(got), flat(ref)):
        err = float((a - b).abs().max() / b.abs().max())
        assert err <= 2e-5, f"{nm}: samples-per-wave vs rays-per-wave {err:.3e}"
    if n_rays <= 4096:
        forced_oracle_check(f"transposed march {n_rays} rays C={C} S={S}", d, dev, chunk=n_rays if rich else 2048, march_order="samples")


def test_march_order_auto_picks_by_ray_coherence():
    """config.march_order = "auto": pinhole images march rays per wavefront, random rays samples per wavefront; decided with the
    check_inputs sync, never when check_inputs is off; both give the oracle's gradients."""
    from lightplane_amd.renderer import check_inputs_and_choose_march
    from tests.synth import random_rays
    dev = _dev()
    gen = torch.Generator().manual_seed(3)
    img = pinhole_rays(128, 128, enc_dim=32, gen=gen).to(dev)
    rnd = random_rays(gen, 1024, 2, 32).to(dev)
    assert lp.config.check_inputs and lp.config.march_order == "auto"
    assert check_inputs_and_choose_march(img, img.grid_idx.int(), 2) == _lib.LP_MARCH_RAYS_PER_WAVE
    assert check_inputs_and_choose_march(rnd, rnd.grid_idx.int(), 2) == _lib.LP_MARCH_SAMPLES_PER_WAVE
    assert check_inputs_and_choose_march(rnd, rnd.grid_idx.int(), 2, "rays") == _lib.LP_MARCH_RAYS_PER_WAVE
    shuffled = img[torch.randperm(img.n_rays, generator=gen).to(dev)]   # random PIXELS of one camera: same origin, unrelated directions
    assert check_inputs_and_choose_march(shuffled, shuffled.grid_idx.int(), 2) == _lib.LP_MARCH_SAMPLES_PER_WAVE
    try:
        lp.config.check_inputs = False
        assert check_inputs_and_choose_march(rnd, rnd.grid_idx.int(), 2) == _lib.LP_MARCH_RAYS_PER_WAVE
    finally:
        lp.config.check_inputs = True
    d = _random_ray_case(2048, 16, 64, seed=5)
    got = run_hip_renderer(d, dev, _lib.LP_KERNEL_AUTO)          # auto -> samples per wavefront
    ref = run_hip_renderer(d, dev, _lib.LP_KERNEL_AUTO, march_order="rays")
    for a, b in zip([got[1], got[2]] + list(got[3]), [ref[1], ref[2]] + list(ref[3])):
        assert float((a - b).abs().max() / b.abs().max()) <= 2e-5


@pytest.mark.parametrize("n_rays,C,S,tri,mask,n_inf", [(4096, 64, 96, False, True, 0), (3000, 32, 70, False, False, 3), (2000, 16, 40, True, True, 0),
                                                        (70000, 32, 33, False, False, 0), (500, 64, 20, True, False, 0)],
                         ids=["refbench_like_c64_s96_mask", "voxel_c32_s70_inf3", "triplane_c16_s40_mask", "70k_rays_voxel_c32_s33", "triplane_c64_s20_short_march"])
def test_splatter_transposed_march_on_random_rays(n_rays, C, S, tri, mask, n_inf):
    """The Splatter's forward walk with march_order="samples" (one ray x 32 consecutive samples per wavefront: the atomic walk merges
    along the ray) on batches of unrelated rays -- the reference's splatter_speed_benchmark.py kind of input: the normalised output
    grids and grad_encoding against march_order="rays" (same arithmetic per (ray, sample), another summation order) and, for the
    small cases, against the oracle.  Voxel (carried columns, weight windows) and plane walks, 16 / 32 / 64 channels, ragged last
    blocks, beyond-far samples, a march shorter than one block."""
    from tests.synth import random_rays
    dev = _dev()
    gen = torch.Generator().manual_seed(n_rays % 89)
    B, G = 2, 24
    sizes = grid_sizes_for((B, G, G + 2, G - 4, C), tri)
    rays = random_rays(gen, n_rays, B, None)
    rays.encoding = torch.rand(n_rays, C, generator=gen)
    up = [torch.randn(*s, generator=gen) for s in sizes]
    cfg = dict(num_samples=S, num_samples_inf=n_inf, mask_out_of_bounds_samples=mask, contract_coords=n_inf > 0)

    def run(order):
        r = rays.to(dev)
        r.encoding = r.encoding.clone().requires_grad_(True)
        out = lp.lightplane_splatter(r, sizes, march_order=order, **cfg)
        sum((o * u.to(dev)).sum() for o, u in zip(out, up)).backward()
        return out, r.encoding.grad

    ref_out, ref_ge = run("rays")
    got_out, got_ge = run("samples")
    for i, (a, b) in enumerate(zip(got_out, ref_out)):
        _assert_close(f"splat out{i}: samples-per-wave vs rays-per-wave", a, b.detach().cpu().numpy(), tol=2e-5)
    _assert_close("grad_encoding: samples-per-wave vs rays-per-wave", got_ge, ref_ge.cpu().numpy(), tol=2e-5)
    if n_rays <= 4096:
        r = copy.copy(rays)
        r.encoding = rays.encoding.clone().requires_grad_(True)
        o_out = O.lightplane_splatter_naive(r, sizes, **cfg)
        sum((o * u).sum() for o, u in zip(o_out, up)).backward()
        for i, (a, b) in enumerate(zip(got_out, o_out)):
            _assert_close(f"splat out{i} vs oracle", a, b.detach().numpy())
        _assert_close("grad_encoding vs oracle", got_ge, r.encoding.grad.numpy())


@pytest.mark.parametrize("H,W,C,tri,S", [(64, 64, 16, True, 24), (50, 72, 32, False, 20), (135, 96, 16, True, 40), (256, 256, 16, True, 128)],
                         ids=["64x64_triplane", "50x72_voxel_tail_rows", "135x96_segmented", "cfg2_image"])
def test_row_length_hint_gives_the_same_rays_their_same_results(H, W, C, tri, S):
    """LpRays.row_length (rays_per_row / auto-detected): the Splatter's backward walk deals 2 x 4 pixel patches to a wavefront
    instead of 8 pixels of one row; the Renderer accepts the hint and ignores it (profiles/r06_ray_order.txt).  Per-ray results do
    not depend on it: Renderer outputs BIT-IDENTICAL, gradients equal up to the order of the fp32 atomics.  Image heights that are no
    multiple of four (the last rows keep their scanline order), a segmented small batch, the headline image; detection by the
    front-end."""
    from lightplane_amd.renderer import check_inputs_and_plan
    dev = _dev()
    gen = torch.Generator().manual_seed(H + W)
    sizes = grid_sizes_for((1, 20, 24, 28, C), tri) if S < 100 else grid_sizes_for((1, 64, 64, 64, C), True)
    grids = random_grids(gen, sizes)
    dec = random_decoder(gen, 2, 2, 2, C, 32, 3, std=0.2)
    rays = pinhole_rays(H, W, enc_dim=32, gen=gen, azimuth_deg=25.0, elevation_deg=20.0)
    n = rays.n_rays
    up = (torch.randn(n, generator=gen), torch.randn(n, generator=gen), torch.randn(n, 3, generator=gen))
    cfg = dict(num_samples=S, gain=1.0, num_samples_inf=0, mask_out_of_bounds_samples=False, contract_coords=False, inject_noise_sigma=0.0,
               inject_noise_seed=0)
    d = dict(rays=rays, grids=grids, color_grids=None, decoder=dec, scaffold=None, cfg=cfg, sizes=sizes, upstream=up)
    assert check_inputs_and_plan(rays.to(dev), rays.grid_idx.int().to(dev), 1) == (_lib.LP_MARCH_RAYS_PER_WAVE, W)   # detected
    ref = run_hip_renderer(d, dev, _lib.LP_KERNEL_AUTO, rays_per_row=0)
    got = run_hip_renderer(d, dev, _lib.LP_KERNEL_AUTO, rays_per_row=W)
    auto = run_hip_renderer(d, dev, _lib.LP_KERNEL_AUTO)
    for a, b, c in zip(got[0], ref[0], auto[0]):
        assert torch.equal(a, b) and torch.equal(c, b)
    for nm, a, b in [("grad_mlp_params", got[1], ref[1]), ("grad_encoding", got[2], ref[2])] + [(f"grad_grid{i}", x, y) for i, (x, y) in enumerate(zip(got[3], ref[3]))]:
        err = float((a - b).abs().max() / b.abs().max())
        assert err <= 2e-5, f"{nm}: with vs without the row-length hint {err:.3e}"
    # the Splatter: forward unchanged, backward walk with 2 x 4 pixel patches
    srays = pinhole_rays(H, W, gen=gen, azimuth_deg=25.0, elevation_deg=20.0)
    srays.encoding = torch.rand(n, C, generator=gen)
    ssz = [[1, 18, 20, 16, C]]
    sup = torch.randn(*ssz[0], generator=gen).to(dev)

    def splat(row):
        r = srays.to(dev)
        r.encoding = r.encoding.clone().requires_grad_(True)
        (out,) = lp.lightplane_splatter(r, ssz, num_samples=S, rays_per_row=row)
        (out * sup).sum().backward()
        return out, r.encoding.grad

    o0, g0 = splat(0)
    o1, g1 = splat(W)
    _assert_close("splat out", o1, o0.detach().cpu().numpy(), tol=2e-5)
    _assert_close("splat grad_encoding", g1, g0.cpu().numpy(), tol=2e-5)


# ---------------------------------------------------------------------------------------------------------------------
# MLP-Splatter at full-chip batches: the forced-oracle proof on the launches only batches of this size select
# ---------------------------------------------------------------------------------------------------------------------
def _mlp_splatter_scale_inputs(H, W, n_layers, hidden, E, CO, out_base, triplane, in_base, S, S_inf=0, mask=False, contract=False, seed=0):
    """A pinhole image of H x W rays (one batch entry) through an MLP [E, hidden x (n_layers - 1), CO] splatted into an output grid
    of ``out_base`` (voxel or triplane), reading a voxel input grid of ``in_base``; in the layout of tests.synth.SplatterCase.build()."""
    from tests.synth import random_splatter_mlp
    gen = torch.Generator().manual_seed(seed)
    rays = pinhole_rays(H, W, cam_dist=2.4, enc_dim=E, gen=gen, azimuth_deg=30.0, elevation_deg=20.0)
    rays.encoding = torch.rand(rays.n_rays, E, generator=gen)
    out_sizes = grid_sizes_for(list(out_base[:4]) + [CO], triplane)
    in_sizes = grid_sizes_for(list(in_base[:4]) + [E], False)
    in_grids = random_grids(gen, in_sizes)
    mlp = random_splatter_mlp(gen, n_layers, E, hidden, CO, std=0.2)
    cfg = dict(num_samples=S, num_samples_inf=S_inf, mask_out_of_bounds_samples=mask, contract_coords=contract)
    up = [torch.randn(*s, generator=gen) for s in out_sizes]
    return dict(rays=rays, out_sizes=out_sizes, mlp=mlp, in_grids=in_grids, in_sizes=in_sizes, cfg=cfg, upstream=up)


# name: (image H, W, layers, hidden, E, CO, output grid, triplane, input grid, samples, beyond-far samples, mask, contract, kernel,
#        the launch it has to reach: (family, forward waves per workgroup, backward segments, backward instantiation, blocks))
MLP_SPLAT_SCALE_CASES = {
    # the reference sweep's shape at 65 536 rays: eight-wave forward, one-sweep two-block backward (two-limb bf16 dW)
    "voxel_3x64_e64_co32_65k": (256, 256, 3, 64, 64, 32, (1, 40, 40, 40), False, (1, 24, 24, 24), 16, 11, False, True,
                                _lib.LP_KERNEL_AUTO, (3, 8, 1, 4, 2)),
    "triplane_4x64_e32_co16_65k": (256, 256, 4, 64, 32, 16, (1, 64, 64, 64), True, (1, 24, 24, 24), 16, 11, True, False,
                                   _lib.LP_KERNEL_AUTO, (3, 8, 1, 4, 2)),
    # LightplaneMLPSplatter's default depth: the two-layer backward at two waves per SIMD
    "voxel_2x32_e32_co32_s64_65k": (256, 256, 2, 32, 32, 32, (1, 40, 40, 40), False, (1, 24, 24, 24), 64, 0, False, False,
                                    _lib.LP_KERNEL_AUTO, (3, 4, 1, 2, 1)),
    # a small batch of long rays: the segmented backward
    "voxel_3x64_e64_co32_s96_1k": (32, 32, 3, 64, 64, 32, (1, 40, 40, 40), False, (1, 24, 24, 24), 96, 0, True, False,
                                   _lib.LP_KERNEL_AUTO, (3, 4, 6, 4, 2)),
    # the shape-generic kernels at 16 384 rays
    "generic_voxel_3x64_e64_co32_16k": (128, 128, 3, 64, 64, 32, (1, 40, 40, 40), False, (1, 24, 24, 24), 16, 11, False, True,
                                        _lib.LP_KERNEL_GENERIC, (0, 1, 1, 0, 0)),
}


@pytest.mark.filterwarnings("ignore:The splatter has been configured")
@pytest.mark.parametrize("name", list(MLP_SPLAT_SCALE_CASES), ids=list(MLP_SPLAT_SCALE_CASES))
def test_mlp_splatter_forced_proof_at_scale(name):
    """The MLP-Splatter at the batch sizes that select its full-chip launches (asserted through lp_mlp_splatter_launch_shape): the
    production backward's ReLU decisions forced onto the chunked fp64 oracle, every forced unit a near tie, every output and every
    gradient entry -- grad_mlp_params summed over every sample of every ray included -- within 1e-4 outright."""
    from lightplane_amd.splatter import mlp_splatter_launch_shape
    from tests.test_gpu_parity import forced_oracle_check_mlp_splatter
    H, W, L, hid, E, CO, ob, tri, ib, S, S_inf, mask, contract, kernel, want = MLP_SPLAT_SCALE_CASES[name]
    d = _mlp_splatter_scale_inputs(H, W, L, hid, E, CO, ob, tri, ib, S, S_inf, mask, contract)
    shape = mlp_splatter_launch_shape(d["rays"].n_rays, d["out_sizes"], d["mlp"], d["in_sizes"], S, S_inf, kernel=kernel)
    got = (shape["family"], shape["fwd_waves"], shape["bwd_segments"], shape["bwd_layers"], shape["blocks"])
    assert got == want, f"{name}: launch {shape}, this test is meant for {want}"
    forced_oracle_check_mlp_splatter(name, d, _dev(), kernel=kernel)

"""GPU parity on IMAGE-COHERENT rays (pinhole cameras) and at BASELINE-config scale.

The golden / sweep cases draw <=130 unrelated rays on grids of <=20 cells: consecutive rays almost never share a
cell there.  The production kernels' most intricate code -- the run-merged gradient scatter of the Renderer backward
(lp_mfma_common.h scatter_plane_ax / scatter_grid), the voxel column walk with carried columns and the 16-cell weight
window of the Splatter (lp_splat_walk.h), splat_bwd_walk_kernel -- only does something when CONSECUTIVE rays share or
neighbour a cell.  These tests render / splat whole pinhole images (row-major pixel order, several rays per cell, dead
rays inside runs through mask_out_of_bounds_samples) and hold every output and every gradient family to the CPU oracle
(reference: tests/test_renderer_with_autograd.py:134-268, tests/test_splatter_with_autograd.py:37-279 run the same
differential on random rays).

Bars: max |err| / max |ref| <= 1e-4 per tensor (north_star) against the fp32 oracle AND a relative L2 error <= 1e-4 (many
small wrong entries of a sparse gradient cannot hide behind the tensor's largest one).

ReLU-flip allowance (gradients only).  The gradient of a ReLU network is a discontinuous function of its inputs: a
pre-activation within round-off of zero takes the other branch when the summation order changes.  With ~10^5 samples x
128 hidden units per test a handful of such flips between ANY two fp32 evaluations is certain -- the fp32 oracle itself
differs from the same oracle run in fp64 by up to 6e-2 of the largest entry on a few cells of these very cases (measured:
4e-3 .. 6e-2 on grad_grid, 5e-4 on grad_encoding, on 1 .. 3 rays), and nothing can reproduce that bit pattern except the
reference's exact summation order.  A flipped unit touches the taps of ONE sample (<= 12 rows x C entries of grad_grid, one
ray of grad_encoding, one row / column of a weight matrix).  So a gradient tensor that misses the 1e-4 bar still passes if
the misses look like that: at most FLIP_SAMPLES samples' worth of entries above the bar, none above 5e-2 of the largest
entry, relative L2 error <= 1e-3.  A dropped or misplaced run of the scatter walk fails all three (the bug this file found
in scatter_plane_ax: 64 entries off by 10-40 %, relative L2 3e-2); outputs never get the allowance.
"""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib
from oracle import lightplane_oracle as O
from tests.synth import (cat_rays, grid_sizes_for, pinhole_crop, pinhole_rays, random_decoder, random_grids,
                         random_splatter_mlp)
from tests.test_gpu_parity import (KERNEL_IDS, KERNELS, TieMasks, _assert_close, _dev, _rel_err, assert_grad_close, forced_oracle_check,
                                   has_dump_twin, rel_l2, run_hip_mlp_splatter, run_hip_renderer, run_hip_splatter, run_oracle_renderer)

pytestmark = pytest.mark.gpu
F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_renderer64(d):
    rays = copy.copy(d["rays"])
    for f in ("directions", "origins", "near", "far", "encoding"):
        setattr(rays, f, getattr(rays, f).to(F64))
    rays.encoding = rays.encoding.clone().requires_grad_(True)
    dec = copy.copy(d["decoder"])
    dec.mlp_params = dec.mlp_params.to(F64).clone().requires_grad_(True)
    grids = [g.to(F64).clone().requires_grad_(True) for g in d["grids"]]
    cgrids = None if d["color_grids"] is None else [g.to(F64).clone().requires_grad_(True) for g in d["color_grids"]]
    scaffold = None if d["scaffold"] is None else d["scaffold"].to(F64)
    out = O.lightplane_renderer_naive(rays, grids, dec, scaffold=scaffold, color_grid=cgrids, **d["cfg"])
    g_len, g_nlt, g_feat = (u.to(F64) for u in d["upstream"])
    ((out[0] * g_len).sum() + (out[1] * g_nlt).sum() + (out[2] * g_feat).sum()).backward()
    return out, dec.mlp_params.grad, rays.encoding.grad, [g.grad for g in grids], None if cgrids is None else [g.grad for g in cgrids]


# --------------------------------------------------------------------------------------------------------------
# Renderer, coherent rays
# --------------------------------------------------------------------------------------------------------------

IMAGES = {
    # name: (height, width, azimuth, elevation)
    "64x64_axis": (64, 64, 0.0, 0.0),
    "48x80_az30_el45": (48, 80, 30.0, 45.0),  # 80 is not a multiple of 32: runs straddle image rows inside a wave
}
BIG_IMAGE = {"128x128_az20_el30": (128, 128, 20.0, 30.0)}  # segmented-backward test only (16 384 rays)
GRIDS = {
    # name: (base, triplane, extra_voxel, separate colour grid, n_layers, batch)
    "triplane24_c16": ((1, 24, 24, 24, 16), True, False, False, (2, 2, 2), 1),
    "voxel20_c32": ((1, 20, 20, 20, 32), False, False, False, (2, 2, 2), 1),
    "triplane_plus_voxel_c16": ((1, 24, 24, 24, 16), True, True, False, (2, 2, 2), 1),
    "two_grid_triplane_c16": ((1, 24, 24, 24, 16), True, False, True, (0, 2, 2), 1),
    "voxel18_c16_b2": ((2, 18, 16, 20, 16), False, False, False, (2, 2, 2), 2),
    # 64 grid channels: the looped family's two-block instantiation, four channels per lane in the run-merged scatter
    "triplane24_c64": ((1, 24, 24, 24, 64), True, False, False, (2, 2, 2), 1),
    "voxel16_c64": ((1, 16, 16, 16, 64), False, False, False, (2, 1, 2), 1),
    # the reference example's decoder depth (1 trunk layer, opacity head without hidden layer, colour head with one): with
    # hidden=64 the two-block looped kernels' one-trunk-layer instantiations
    "triplane24_c32_t1o1c2": ((1, 24, 24, 24, 32), True, False, False, (1, 1, 2), 1),
    "voxel20_c16_t1o1c2": ((1, 20, 20, 20, 16), False, False, False, (1, 1, 2), 1),
}
# deep decoders (layer-looped MFMA family, lp_renderer_loop.hip): test_renderer_coherent_deep
DEEP_GRIDS = {
    "triplane24_c16_deep444": ((1, 24, 24, 24, 16), True, False, False, (4, 4, 4), 1),
    "voxel20_c32_deep342": ((1, 20, 20, 20, 32), False, False, False, (3, 4, 2), 1),
    "two_grid_mixed_c16_deep044": ((1, 24, 24, 24, 16), True, True, True, (0, 4, 4), 1),
}


def coherent_renderer_inputs(grid_name, image_name, mask_oob=True, num_samples=24, seed=0, hidden=32, color_chn=3,
                             scaffold=False):
    base, tri, extra, sep, n_layers, batch = {**GRIDS, **DEEP_GRIDS}[grid_name]
    height, width, az, el = {**IMAGES, **BIG_IMAGE}[image_name]
    gen = torch.Generator().manual_seed(seed)
    B, C = base[0], base[-1]
    sizes = grid_sizes_for(base, tri)
    if extra:
        sizes = sizes + [[B, 12, 10, 14, C]]
    grids = random_grids(gen, sizes)
    cgrids = random_grids(gen, sizes) if sep else None
    dec = random_decoder(gen, *n_layers, input_chn=C, hidden_chn=hidden, color_chn=color_chn,
                         use_separate_color_grid=sep, std=0.2)
    enc_dim = int(dec.n_hidden_color[0])
    parts = []
    for b in range(batch):  # one camera image per batch entry, from different sides
        parts.append(pinhole_rays(height, width, enc_dim=enc_dim, gen=gen, grid_idx=b, azimuth_deg=az + 70.0 * b,
                                  elevation_deg=el - 20.0 * b))
    rays = parts[0] if batch == 1 else cat_rays(parts)
    n = rays.n_rays
    sc = None
    if scaffold:
        sc = (torch.rand(B, 7, 6, 8, generator=gen) > 0.35).float()
    cfg = dict(num_samples=num_samples, gain=2.0, num_samples_inf=0, mask_out_of_bounds_samples=mask_oob,
               contract_coords=False, inject_noise_sigma=0.0, inject_noise_seed=0)
    up = (torch.randn(n, generator=gen), torch.randn(n, generator=gen), torch.randn(n, color_chn, generator=gen))
    return dict(rays=rays, grids=grids, color_grids=cgrids, decoder=dec, scaffold=sc, cfg=cfg, sizes=sizes, upstream=up)


def check_renderer(d, dev, kernel, tag, **extra):
    """Outputs against the fp32 oracle at 1e-4.  Gradients: where the kernel that runs has a DUMP twin (every family since round 6,
    the shape-generic kernels included) the PROOF -- its own ReLU decisions forced onto the fp64 oracle, every forced unit a measured
    near tie, every entry at 1e-4 (forced_oracle_check); the counted allowance of assert_grad_close is left to early termination."""
    if has_dump_twin(d, kernel=kernel, **extra):
        out = run_hip_renderer(d, dev, kernel, **extra)[0]
        o_out = run_oracle_renderer(d)[0]
        for nm, a, b in (("ray_length", out[0], o_out[0]), ("neg_log_t", out[1], o_out[1]), ("feature", out[2], o_out[2])):
            _assert_close(f"{tag}: {nm}", a, b.detach().numpy())
        forced_oracle_check(tag, d, dev, chunk=2048 if d["cfg"]["inject_noise_sigma"] == 0 else d["rays"].n_rays, kernel=kernel, **extra)
        return
    out, gp, ge, gg, gc = run_hip_renderer(d, dev, kernel, **extra)
    o_out, o_gp, o_ge, o_gg, o_gc = run_oracle_renderer(d)       # the reference's arithmetic (fp32)
    for nm, a, b in (("ray_length", out[0], o_out[0]), ("neg_log_t", out[1], o_out[1]), ("feature", out[2], o_out[2])):
        _assert_close(f"{tag}: {nm}", a, b.detach().numpy())
    C = d["grids"][0].shape[-1]
    width = max(int(v) for v in list(d["decoder"].n_hidden_trunk) + list(d["decoder"].n_hidden_color))
    q = []

    def oracle64():  # the second oracle of the flip allowance: run once, only when some tensor misses the bar
        if not q:
            q.append(oracle_renderer64(d))
        return q[0]

    ties = TieMasks(d)  # where a near-tie ReLU can reach: the only places an entry may miss BOTH oracles
    assert_grad_close(f"{tag}: grad_mlp_params", gp, o_gp.numpy(), 4 * width, want64=lambda: oracle64()[1].numpy(),
                      tie_mask=ties.params_mask())
    assert_grad_close(f"{tag}: grad_encoding", ge, o_ge.numpy(), ge.shape[1], want64=lambda: oracle64()[2].numpy(),
                      tie_mask=ties.encoding_mask())
    for i, (a, b) in enumerate(zip(gg, o_gg)):
        assert_grad_close(f"{tag}: grad_grid{i}", a, b.numpy(), 8 * C, want64=lambda i=i: oracle64()[3][i].numpy(),
                          tie_mask=ties.grid_mask(i))
    if gc is not None:
        for i, (a, b) in enumerate(zip(gc, o_gc)):
            assert_grad_close(f"{tag}: grad_color_grid{i}", a, b.numpy(), 8 * C, want64=lambda i=i: oracle64()[4][i].numpy(),
                              tie_mask=ties.color_grid_mask(i))


@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("image", list(IMAGES))
@pytest.mark.parametrize("grid", list(GRIDS))
def test_renderer_coherent_image(grid, image, kernel):
    """Whole pinhole images (several rays per cell, masked samples inside runs): outputs + all gradient families."""
    d = coherent_renderer_inputs(grid, image)
    check_renderer(d, _dev(), kernel, f"{grid}/{image}")


@pytest.mark.parametrize("grid,kw", [
    ("triplane24_c16", dict(mask_oob=False)),                       # unmasked: border cells re-expressed in the plane walk
    ("voxel20_c32", dict(mask_oob=False, color_chn=4)),              # 4 colour channels: NC = 4 instantiations
    ("triplane24_c16", dict(scaffold=True)),                        # non-PLAIN instantiation, occupancy zeros inside runs
    ("voxel20_c32", dict(hidden=16, mask_oob=True)),                 # flex family (hidden 16 padded to 32)
    ("triplane_plus_voxel_c16", dict(hidden=64, mask_oob=True)),     # hidden 64 (two-block looped kernels)
    ("triplane24_c32_t1o1c2", dict(hidden=64)),                      # the reference example's 1/1/2 x 64: two-block looped, one trunk layer
    ("voxel20_c16_t1o1c2", dict(hidden=64, scaffold=True)),          # the same on 16 channels, non-PLAIN
    ("two_grid_triplane_c16", dict(hidden=64)),                      # two-grid decoder x 64 (two-block looped kernels since 0.2.4)
], ids=["triplane_nomask", "voxel_nomask_rgba", "triplane_scaffold", "voxel_flex_h16", "mixed_h64", "example_112_h64_c32", "example_112_h64_c16",
        "two_grid_h64"])
def test_renderer_coherent_variants(grid, kw):
    d = coherent_renderer_inputs(grid, "48x80_az30_el45", seed=3, **kw)
    check_renderer(d, _dev(), _lib.LP_KERNEL_AUTO, f"{grid}/{kw}")


@pytest.mark.parametrize("grid,kw", [
    ("triplane24_c16_deep444", dict()),
    ("voxel20_c32_deep342", dict(mask_oob=False, color_chn=4)),
    ("two_grid_mixed_c16_deep044", dict(scaffold=True)),
    ("triplane24_c16_deep444", dict(hidden=16, mask_oob=False)),
], ids=["triplane_444", "voxel_342_rgba", "two_grid_044_scaffold", "triplane_444_h16"])
def test_renderer_coherent_deep(grid, kw):
    """Whole pinhole images through the layer-looped MFMA family (3-4 layers per MLP): run-merged scatter, workgroup-shared dW
    of ten layers, the two-grid decoder's colour-grid scatter."""
    d = coherent_renderer_inputs(grid, "48x80_az30_el45", seed=5, **kw)
    assert lp.kernel_family(d["rays"], d["grids"], d["decoder"], color_grid=d["color_grids"]) == 3
    check_renderer(d, _dev(), _lib.LP_KERNEL_AUTO, f"{grid}/{kw}")


def test_loop_family_on_the_shapes_of_the_other_families():
    """LP_LOOP=1 (read once per process) sends every shape the layer-looped family supports through it -- also the default
    2/2/2 x 32 shape, the flex shapes, hidden 64 and the two-layer MLP-Splatter: the golden suite and a coherent image in a
    child process."""
    env = dict(os.environ, LP_LOOP="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests"), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "renderer_matches or mlp_splatter_matches or test_renderer_coherent_image"],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1200)
    assert r.returncode == 0, r.stdout.decode()[-3000:]


def test_renderer_coherent_early_termination_exact_when_off():
    """stop_transmittance = 0 on coherent rays is the exact kernel (non-PLAIN bookkeeping with on-flags)."""
    d = coherent_renderer_inputs("triplane24_c16", "64x64_axis", seed=5)
    d["cfg"] = dict(d["cfg"], num_samples_inf=2)  # non-PLAIN instantiation
    check_renderer(d, _dev(), _lib.LP_KERNEL_AUTO, "triplane/inf2")


# --------------------------------------------------------------------------------------------------------------
# segment-parallel backward of small batches (LpRendererArgs.seg_prefix)
# --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("grid,num_samples,kw", [
    ("triplane24_c16", 88, dict()),                                # 6 segments, ragged last one (8 samples)
    ("triplane24_c16", 64, dict(mask_oob=False)),                  # 4 full segments
    ("triplane24_c16", 33, dict()),                                # third segment = a single sample
    ("triplane_plus_voxel_c16", 72, dict()),                       # run-time grid-list loop
    ("voxel18_c16_b2", 96, dict(color_chn=4)),                     # NC = 4: the fourth colour sum lives in the second float4
    ("triplane24_c16", 70, dict(scaffold=True, noise=True)),       # non-PLAIN instantiation
    ("triplane24_c16", 80, dict(image="128x128_az20_el30")),       # 128 ray blocks x 5 states > 512: segments of 32, 32, 16
    ("voxel20_c32", 72, dict()),                                   # C = 32 instantiations
    ("voxel20_c32", 50, dict(hidden=16)),                          # flex family (fp32-MFMA kernels, run-time segment switch)
    ("two_grid_triplane_c16", 66, dict()),                         # two-grid decoder: second scatter per sample
    ("triplane_plus_voxel_c16", 50, dict(hidden=64)),              # hidden 64 (two-block looped kernels)
    ("voxel20_c32", 40, dict(hidden=64, scaffold=True)),           # hidden 64 (two-block looped kernels), C = 32, non-PLAIN
    ("two_grid_triplane_c16", 66, dict(hidden=64)),                # two-grid decoder x 64
    ("triplane24_c16_deep444", 72, dict()),                        # layer-looped family: ragged last segment
    ("voxel20_c32_deep342", 50, dict(scaffold=True, noise=True, color_chn=4)),  # layer-looped family, C = 32, fourth colour sum
    ("two_grid_mixed_c16_deep044", 66, dict()),                    # layer-looped two-grid decoder
], ids=["triplane_s88", "triplane_s64_nomask", "triplane_s33", "mixed_s72", "voxel_b2_rgba_s96", "triplane_scaffold_noise_s70",
        "triplane_16k_rays_s80", "voxel_c32_s72", "voxel_flex_h16_s50", "two_grid_s66", "mixed_h64_s50", "voxel_c32_h64_scaffold_s40", "two_grid_h64_s66",
        "deep444_s72", "deep342_c32_scaffold_noise_s50", "deep_two_grid_s66"])
def test_segmented_backward(grid, num_samples, kw):
    """4 096-ray image, S > 16: the backward runs one workgroup per (128 rays, one or two blocks of LP_SEG_LEN = 8 samples) and has to agree with
    the oracle AND with the one-workgroup-per-128-rays sweep of the same kernel (same recompute, so no ReLU-flip slack:
    1e-5 of the largest entry)."""
    dev = _dev()
    kw = dict(kw)
    noise = kw.pop("noise", False)
    image = kw.pop("image", "64x64_axis")
    # (seed 11 puts one ReLU pre-activation of the S = 33 case within round-off of zero: a single flipped sample, 62 entries
    # per plane up to 2.9e-2 / relative L2 3e-3 between the kernel and the fp32 oracle -- scripts/diag_s33.py)
    d = coherent_renderer_inputs(grid, image, num_samples=num_samples, seed=3 if num_samples == 33 else 11, **kw)
    if noise:
        d["cfg"] = dict(d["cfg"], inject_noise_sigma=0.3, inject_noise_seed=5)
    n_seg = -(-num_samples // _lib.LP_SEG_LEN)
    assert lp.backward_segments(d["rays"], d["grids"], d["decoder"], color_grid=d["color_grids"], **d["cfg"]) == n_seg
    assert lp.config.segment_backward
    try:
        lp.config.segment_backward = False
        ref = run_hip_renderer(d, dev, _lib.LP_KERNEL_AUTO)
    finally:
        lp.config.segment_backward = True
    got = run_hip_renderer(d, dev, _lib.LP_KERNEL_AUTO)
    for a, b in zip(got[0], ref[0]):
        assert torch.equal(a, b)  # the same (segmented) forward in both runs
    # the segmented forward (one workgroup per segment + combine pass) against the single march: rounding only
    try:
        lp.config.segment_forward = False
        single = run_hip_renderer(d, dev, _lib.LP_KERNEL_AUTO)
    finally:
        lp.config.segment_forward = True
    for nm, a, b in zip(("ray_length", "neg_log_t", "feature"), got[0], single[0]):
        err = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)
        assert err <= 2e-6, f"{nm}: segmented forward vs single march {err:.3e}"
    with torch.no_grad():  # inference: no gradient state, still segmented
        rays = d["rays"].to(dev)
        dec = d["decoder"]
        hdec = lp.DecoderParams(dec.mlp_params.to(dev), dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
        out = lp.lightplane_renderer(rays, [g.to(dev) for g in d["grids"]], hdec,
                                     color_grid=None if d["color_grids"] is None else [g.to(dev) for g in d["color_grids"]],
                                     scaffold=None if d["scaffold"] is None else d["scaffold"].to(dev), **d["cfg"])
    for a, b in zip(out, got[0]):
        assert torch.equal(a, b.detach())
    flat = lambda r: [r[1], r[2]] + list(r[3]) + list(r[4] or [])
    for i, (a, b) in enumerate(zip(flat(got), flat(ref))):
        err = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)
        assert err <= 1e-5, f"gradient tensor {i}: segmented vs single sweep {err:.3e}"
    check_renderer(d, dev, _lib.LP_KERNEL_AUTO, f"segmented {grid}/S={num_samples}")


@pytest.mark.parametrize("alpha_mode", [1, 2])
def test_segmented_march_with_fused_epilogue(alpha_mode):
    """Background compositing + alpha written by the combine pass of the segmented forward, their gradients folded into the
    segmented backward: against the single march / single sweep of the same kernels."""
    from lightplane_amd.renderer import _render
    dev = _dev()
    d = coherent_renderer_inputs("triplane24_c16", "64x64_axis", num_samples=56, seed=7)
    gen = torch.Generator().manual_seed(1)
    n = d["rays"].n_rays
    up = [torch.randn(n, generator=gen).to(dev), torch.randn(n, generator=gen).to(dev),
          torch.randn(n, 3, generator=gen).to(dev), torch.randn(n, generator=gen).to(dev)]
    bg = torch.tensor([0.2, 0.7, 0.4], device=dev)

    def run():
        rays = d["rays"].to(dev)
        rays.encoding = rays.encoding.clone().requires_grad_(True)
        dec = d["decoder"]
        params = dec.mlp_params.to(dev).clone().requires_grad_(True)
        hdec = lp.DecoderParams(params, dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
        grids = [g.to(dev).clone().requires_grad_(True) for g in d["grids"]]
        out = _render(rays, grids, hdec, bg_color=bg, alpha_mode=alpha_mode, **d["cfg"])
        sum((o * u).sum() for o, u in zip(out, up)).backward()
        return [o.detach() for o in out], [params.grad, rays.encoding.grad] + [g.grad for g in grids]

    out1, g1 = run()
    try:
        lp.config.segment_forward = lp.config.segment_backward = False
        out0, g0 = run()
    finally:
        lp.config.segment_forward = lp.config.segment_backward = True
    for i, (a, b) in enumerate(zip(out1, out0)):
        err = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)
        assert err <= 2e-6, f"output {i}: {err:.3e}"
    for i, (a, b) in enumerate(zip(g1, g0)):
        err = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)
        assert err <= 2e-5, f"gradient tensor {i}: {err:.3e}"


def test_segmented_backward_is_not_used_where_it_cannot_be():
    d = coherent_renderer_inputs("triplane24_c16", "64x64_axis", num_samples=64)
    q = lambda **over: lp.backward_segments(d["rays"], d["grids"], d["decoder"], **dict(d["cfg"], **over))
    assert q() == 8
    assert q(num_samples=8) == 1
    assert q(num_samples_inf=2) == 1                                                    # beyond-far samples
    d32 = coherent_renderer_inputs("voxel20_c32", "64x64_axis", num_samples=64)        # C = 32: the same kernels
    assert lp.backward_segments(d32["rays"], d32["grids"], d32["decoder"], **d32["cfg"]) == 8
    dflex = coherent_renderer_inputs("triplane24_c16", "64x64_axis", num_samples=64, hidden=16)  # flex family: the same
    assert lp.backward_segments(dflex["rays"], dflex["grids"], dflex["decoder"], **dflex["cfg"]) == 8
    dwide = coherent_renderer_inputs("triplane24_c16", "64x64_axis", num_samples=64, hidden=64)  # hidden 64: the same
    assert lp.backward_segments(dwide["rays"], dwide["grids"], dwide["decoder"], **dwide["cfg"]) == 8
    assert lp.backward_segments(dwide["rays"], dwide["grids"], dwide["decoder"], **dict(dwide["cfg"], num_samples_inf=1)) == 1
    big = pinhole_rays(256, 256, enc_dim=32, gen=torch.Generator().manual_seed(0))      # 65 536 rays fill the chip
    assert lp.backward_segments(big, d["grids"], d["decoder"], **d["cfg"]) == 1


# --------------------------------------------------------------------------------------------------------------
# Splatter / MLP-Splatter, coherent rays
# --------------------------------------------------------------------------------------------------------------

SPLATS = {
    # name: (out_base, triplane, batch)
    "voxel24_c32": ((1, 24, 24, 24, 32), False, 1),
    "triplane32_c16": ((1, 32, 32, 32, 16), True, 1),
    "voxel20_c32_b2": ((2, 20, 18, 22, 32), False, 2),
    "voxel24_c16": ((1, 24, 24, 24, 16), False, 1),
    "voxel18_c64": ((1, 18, 20, 16, 64), False, 1),   # 64 channels: 16-ray waves, two registers per lane in the two-axis walk
}


def coherent_splatter_inputs(name, image_name, mask_oob=True, num_samples=24, seed=0, mlp=None):
    base, tri, batch = SPLATS[name]
    height, width, az, el = {**IMAGES, **BIG_IMAGE}[image_name]
    gen = torch.Generator().manual_seed(seed)
    out_sizes = grid_sizes_for(base, tri)
    C = base[-1]
    feat_dim = C if mlp is None else mlp["feat_dim"]
    parts = [pinhole_rays(height, width, grid_idx=b, azimuth_deg=az + 70.0 * b, elevation_deg=el - 20.0 * b)
             for b in range(batch)]
    rays = parts[0] if batch == 1 else cat_rays(parts)
    rays.encoding = torch.rand(rays.n_rays, feat_dim, generator=gen)
    d = dict(rays=rays, out_sizes=out_sizes, mlp=None, in_grids=None, in_sizes=None,
             cfg=dict(num_samples=num_samples, num_samples_inf=0, mask_out_of_bounds_samples=mask_oob, contract_coords=False))
    if mlp is not None:
        in_sizes = grid_sizes_for((base[0], 10, 12, 14, feat_dim), mlp.get("in_triplane", False))
        d["in_sizes"] = in_sizes
        d["in_grids"] = random_grids(gen, in_sizes)
        d["mlp"] = random_splatter_mlp(gen, mlp.get("n_layers", 2), feat_dim, mlp.get("hidden", 32), C, std=0.2)
    d["upstream"] = [torch.randn(*s, generator=gen) for s in out_sizes]
    return d


def check_splatter(d, dev, tag):
    out, ge = run_hip_splatter(d, dev)
    rays = copy.copy(d["rays"])
    rays.encoding = rays.encoding.clone().requires_grad_(True)
    o_out = O.lightplane_splatter_naive(rays, d["out_sizes"], **d["cfg"])
    sum((o * u).sum() for o, u in zip(o_out, d["upstream"])).backward()
    for i, o in enumerate(out):
        _assert_close(f"{tag}: out{i}", o, o_out[i].detach().numpy())
    _assert_close(f"{tag}: grad_encoding", ge, rays.encoding.grad.numpy())
    num = (ge.detach().double().cpu() - rays.encoding.grad.double()).norm().item()
    assert num / max(rays.encoding.grad.double().norm().item(), 1e-30) <= 1e-4, f"{tag}: grad_encoding relative L2"


def check_mlp_splatter(d, dev, kernel, tag):
    out, ge, gp, gin = run_hip_mlp_splatter(d, dev, kernel)
    rays = copy.copy(d["rays"])
    rays.encoding = rays.encoding.clone().requires_grad_(True)
    mlp = copy.copy(d["mlp"])
    mlp.mlp_params = mlp.mlp_params.clone().requires_grad_(True)
    in_grids = [g.clone().requires_grad_(True) for g in d["in_grids"]]
    o_out = O.lightplane_mlp_splatter_naive(rays, d["out_sizes"], mlp, in_grids, **d["cfg"])
    sum((o * u).sum() for o, u in zip(o_out, d["upstream"])).backward()
    for i, o in enumerate(out):
        _assert_close(f"{tag}: out{i}", o, o_out[i].detach().numpy())
    _assert_close(f"{tag}: grad_encoding", ge, rays.encoding.grad.numpy())
    _assert_close(f"{tag}: grad_mlp_params", gp, mlp.mlp_params.grad.numpy())
    for i, g in enumerate(gin):
        _assert_close(f"{tag}: grad_input_grid{i}", g, in_grids[i].grad.numpy())


@pytest.mark.parametrize("image", list(IMAGES))
@pytest.mark.parametrize("name", list(SPLATS))
@pytest.mark.parametrize("mask", [True, False], ids=["mask", "nomask"])
def test_splatter_coherent_image(name, image, mask):
    """Column walk with carried columns / 16-cell weight windows / per-slot plane walk on pixel-adjacent rays."""
    d = coherent_splatter_inputs(name, image, mask_oob=mask)
    check_splatter(d, _dev(), f"{name}/{image}/mask={mask}")


@pytest.mark.parametrize("seed", list(range(12)))
def test_splatter_random_cameras(seed):
    """The voxel walks' carries under cameras at RANDOM angles to the grid (round 6: two carry axes chosen per wave-sample, weight
    windows carried over y / z steps, segments of interleaved samples): images of 40 x 56 pixels, non-cubic grids, 16 / 32 / 64
    channels, one or two batch entries, with and without the out-of-bounds mask -- outputs and grad_encoding against the oracle."""
    gen = torch.Generator().manual_seed(1000 + seed)
    rnd = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=gen))
    C = (32, 64, 16, 32)[seed % 4]
    batch = 1 + (seed % 3 == 2)
    base = (batch, rnd(10, 26), rnd(10, 26), rnd(10, 26), C)
    out_sizes = grid_sizes_for(base, False)
    parts = [pinhole_rays(40, 56, grid_idx=b, azimuth_deg=float(torch.rand(1, generator=gen)) * 360.0,
                          elevation_deg=float(torch.rand(1, generator=gen)) * 120.0 - 60.0) for b in range(batch)]
    rays = parts[0] if batch == 1 else cat_rays(parts)
    rays.encoding = torch.rand(rays.n_rays, C, generator=gen)
    d = dict(rays=rays, out_sizes=out_sizes, mlp=None, in_grids=None, in_sizes=None,
             cfg=dict(num_samples=rnd(20, 45), num_samples_inf=0, mask_out_of_bounds_samples=bool(seed & 1), contract_coords=False),
             upstream=[torch.randn(*sz, generator=gen) for sz in out_sizes])
    check_splatter(d, _dev(), f"random camera {seed}: grid {base}")


@pytest.mark.parametrize("name", list(SPLATS))
@pytest.mark.parametrize("num_samples", [37, 70])
def test_splatter_segmented_march(name, num_samples):
    """Small batch, more than 32 samples: the march of the voxel walk kernels is cut into segments (one workgroup per
    64 rays and segment; the backward's segments accumulate grad_encoding with atomics)."""
    d = coherent_splatter_inputs(name, "48x80_az30_el45", num_samples=num_samples, seed=2)
    check_splatter(d, _dev(), f"segmented {name}/S={num_samples}")


@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("name,mlp", [
    ("voxel24_c32", dict(feat_dim=32)),
    ("triplane32_c16", dict(feat_dim=16, in_triplane=True)),
    ("voxel20_c32_b2", dict(feat_dim=16)),
], ids=["voxel_32_32", "triplane_16_16", "voxel_b2_16_32"])
def test_mlp_splatter_coherent_image(name, mlp, kernel):
    d = coherent_splatter_inputs(name, "48x80_az30_el45", seed=2, mlp=mlp)
    check_mlp_splatter(d, _dev(), kernel, f"{name}/mlp")


@pytest.mark.parametrize("name,mlp", [
    ("voxel24_c32", dict(feat_dim=32)),
    ("triplane32_c16", dict(feat_dim=16, in_triplane=True)),
], ids=["voxel_32_32", "triplane_16_16"])
def test_mlp_splatter_segmented_march(name, mlp):
    """Small batch, 70 samples: the MLP-Splatter's march is cut into segments (parameter / input-grid gradients are
    atomics anyway, grad_encoding accumulates over the segments)."""
    d = coherent_splatter_inputs(name, "48x80_az30_el45", num_samples=70, seed=4, mlp=mlp)
    check_mlp_splatter(d, _dev(), _lib.LP_KERNEL_AUTO, f"segmented {name}/mlp")


def test_mlp_splatter_eight_wave_forward():
    """MLP-Splatters whose limb images exclude a second four-wave workgroup per CU (three / four 64-wide layers) run their forward
    on eight-wave workgroups when the batch fills the chip (65 536 rays and more); LP_LOOP_FWD_NW8=1 selects them for the small
    golden / sweep cases too, so that the instantiations are held to the oracle (hidden 64, 3 and 4 layers, feature widths
    32 / 64: the reference's own sweep shapes, tests/test_splatter_with_autograd.py:38-53)."""
    env = dict(os.environ, LP_LOOP_FWD_NW8="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_parity.py"),
                        os.path.join(ROOT, "tests", "test_gpu_sweep.py"), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "test_mlp_splatter_matches_oracle_and_golden or test_reference_splatter_sweep_axes"],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1200)
    assert r.returncode == 0, r.stdout.decode()[-3000:]


# --------------------------------------------------------------------------------------------------------------
# BASELINE-config scale
# --------------------------------------------------------------------------------------------------------------


def test_cfg3_scale_splatter_subimage():
    """BASELINE cfg 3 geometry (256x256 camera, 128^3 x 32 voxel grid, S = 256): the FULL GPU splat of the central 64x64
    block of pixels (ray density of the full image) against the oracle of the same rays, plus grad_encoding."""
    gen = torch.Generator().manual_seed(0)
    rays = pinhole_crop(256, 256, 96, 96, 64, 64)
    rays.encoding = torch.rand(rays.n_rays, 32, generator=gen)
    out_sizes = [[1, 128, 128, 128, 32]]
    d = dict(rays=rays, out_sizes=out_sizes,
             cfg=dict(num_samples=256, num_samples_inf=0, mask_out_of_bounds_samples=False, contract_coords=False))
    # upstream gradient only where the splat lands would be the realistic case; a dense one also checks the empty cells
    d["upstream"] = [torch.randn(*out_sizes[0], generator=gen)]
    check_splatter(d, _dev(), "cfg3-subimage")


def test_cfg4_shape_renderer_block():
    """BASELINE cfg 4 shape (1920x1080 camera at elevation 30 deg, triplane 128^2 x 32 ch, S = 256 -> 8 checkpoint
    intervals): a 16 x 32 block of neighbouring pixels vs the oracle, all gradient families."""
    gen = torch.Generator().manual_seed(1)
    sizes = grid_sizes_for((1, 128, 128, 128, 32), True)
    grids = random_grids(gen, sizes)
    dec = random_decoder(gen, 2, 2, 2, 32, 32, 3, std=0.15)
    rays = pinhole_crop(1080, 1920, 532, 944, 16, 32, enc_dim=32, gen=gen, azimuth_deg=45.0, elevation_deg=30.0)
    n = rays.n_rays
    d = dict(rays=rays, grids=grids, color_grids=None, decoder=dec, scaffold=None, sizes=sizes,
             cfg=dict(num_samples=256, gain=1.0, num_samples_inf=0, mask_out_of_bounds_samples=False,
                      contract_coords=False, inject_noise_sigma=0.0, inject_noise_seed=0),
             upstream=(torch.randn(n, generator=gen), torch.randn(n, generator=gen), torch.randn(n, 3, generator=gen)))
    for kernel in (_lib.LP_KERNEL_AUTO,):
        check_renderer(d, _dev(), kernel, "cfg4-block")


def _chain_hip(rays_s, rays_r, dec, out_sizes, S, dev):
    rs = rays_s.to(dev)
    rs.encoding = rs.encoding.clone().requires_grad_(True)
    rr = rays_r.to(dev)
    rr.encoding = rr.encoding.clone().requires_grad_(True)
    params = dec.mlp_params.to(dev).clone().requires_grad_(True)
    hdec = lp.DecoderParams(params, dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
    grid = lp.lightplane_splatter(rs, out_sizes, num_samples=S)
    out = lp.lightplane_renderer(rr, grid, hdec, num_samples=S, gain=1.0)
    return rs, rr, params, grid, out


def test_cfg5_chain_splatter_into_renderer():
    """BASELINE cfg 5 in miniature: several views are splatted into a voxel grid, the normalised grid is rendered from a
    new view, and the loss back-propagates through the render, the normalisation and the splat into the splatted
    features.  Oracle: naive_splatter -> naive_renderer chained the same way.  The small companion of
    tests/test_gpu_config_scale.py::test_cfg5_full_chain_against_oracle (the same chain at the size bench.py times): small enough for
    the full oracle and autograd end to end, it checks what that test checks per box and per ray."""
    dev = _dev()
    gen = torch.Generator().manual_seed(2)
    S = 48
    out_sizes = [[1, 32, 32, 32, 32]]
    views = [pinhole_rays(40, 40, azimuth_deg=a, elevation_deg=e) for a, e in ((0.0, 0.0), (120.0, 25.0), (240.0, -30.0))]
    rays_s = cat_rays(views)
    rays_s.encoding = torch.rand(rays_s.n_rays, 32, generator=gen)
    rays_r = pinhole_rays(36, 60, enc_dim=32, gen=gen, azimuth_deg=60.0, elevation_deg=15.0)
    dec = random_decoder(gen, 2, 2, 2, 32, 32, 3, std=0.2)
    n = rays_r.n_rays
    up = (torch.randn(n, generator=gen), torch.randn(n, generator=gen), torch.randn(n, 3, generator=gen))

    rs, rr, params, grid, out = _chain_hip(rays_s, rays_r, dec, out_sizes, S, dev)
    for g in grid:
        g.retain_grad()
    sum((o * u.to(dev)).sum() for o, u in zip(out, up)).backward()

    o_rs = copy.copy(rays_s)
    o_rs.encoding = rays_s.encoding.clone().requires_grad_(True)
    o_rr = copy.copy(rays_r)
    o_rr.encoding = rays_r.encoding.clone().requires_grad_(True)
    o_dec = copy.copy(dec)
    o_dec.mlp_params = dec.mlp_params.clone().requires_grad_(True)
    o_grid = O.lightplane_splatter_naive(o_rs, out_sizes, num_samples=S)
    for g in o_grid:
        g.retain_grad()
    o_out = O.lightplane_renderer_naive(o_rr, o_grid, o_dec, num_samples=S, gain=1.0)
    sum((o * u).sum() for o, u in zip(o_out, up)).backward()

    _assert_close("chain: splatted grid", grid[0], o_grid[0].detach().numpy())
    for nm, a, b in zip(("ray_length", "neg_log_t", "feature"), out, o_out):
        _assert_close(f"chain: {nm}", a, b.detach().numpy())
    _assert_close("chain: grad_mlp_params", params.grad, o_dec.mlp_params.grad.numpy())
    _assert_close("chain: grad render encoding", rr.encoding.grad, o_rr.encoding.grad.numpy())
    _assert_close("chain: grad of the splatted grid", grid[0].grad, o_grid[0].grad.numpy())
    _assert_close("chain: grad splatted encoding (end to end)", rs.encoding.grad, o_rs.encoding.grad.numpy())


_VARIANT_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, {root!r})
from tests.test_gpu_coherent import coherent_renderer_inputs
from tests.test_gpu_parity import run_hip_renderer
from lightplane_amd import _lib
d = coherent_renderer_inputs({grid!r}, "48x80_az30_el45", seed=7, mask_oob={mask})
out, gp, ge, gg, gc = run_hip_renderer(d, torch.device("cuda:0"), _lib.LP_KERNEL_AUTO)
np.savez({path!r}, ray_length=out[0].detach().cpu().numpy(), neg_log_t=out[1].detach().cpu().numpy(),
         feature=out[2].detach().cpu().numpy())
"""


@pytest.mark.parametrize("grid", ["triplane24_c16", "voxel18_c16_b2", "voxel20_c32"])
@pytest.mark.parametrize("variant", ["bf3_occ2", "bf3_occ3"])
def test_forward_variants_agree(grid, variant, tmp_path):
    """Every forward instantiation the launcher can pick for the default decoder shape gives the oracle's outputs: the
    bf16x3 kernel at 2 / 3 waves per SIMD (LP_BF3_OCC; 3 is what batches above 65 536 rays select, i.e. every 1080p
    batch).  (The fp32-MFMA forward variants this test also covered were retired in round 4.)  The knob is read once per
    process: child processes."""
    path = str(tmp_path / f"v{variant}.npz")
    kind, num = variant.rsplit("_", 1)
    assert kind == "bf3"
    extra = {"LP_BF3_OCC": num[-1]}
    env = dict(os.environ, **extra)
    code = _VARIANT_CHILD.format(root=ROOT, grid=grid, mask=True, path=path)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    z = np.load(path)
    d = coherent_renderer_inputs(grid, "48x80_az30_el45", seed=7, mask_oob=True)
    o_out = O.lightplane_renderer_naive(d["rays"], d["grids"], d["decoder"], **d["cfg"])
    for nm, o in zip(("ray_length", "neg_log_t", "feature"), o_out):
        _assert_close(f"variant {variant}: {nm}", torch.from_numpy(z[nm]), o.detach().numpy())


def test_1080p_c16_batch_uses_variant4_and_matches_oracle_subsample():
    """A real 1080p x C = 16 batch (2 073 600 rays: the launcher picks the three-waves-per-SIMD bf16x3 forward, renderer_fwd_bf3<16, GM, 3, 3>): a block
    of 24 x 40 neighbouring pixels of the full-size launch equals the oracle of those rays (per-ray outputs do not
    depend on the batch), S = 32 to keep the launch short."""
    dev = _dev()
    gen = torch.Generator().manual_seed(4)
    sizes = grid_sizes_for((1, 64, 64, 64, 16), True)
    grids = random_grids(gen, sizes)
    dec = random_decoder(gen, 2, 2, 2, 16, 32, 3, std=0.15)
    rays = pinhole_rays(1080, 1920, azimuth_deg=45.0, elevation_deg=30.0)
    rays.encoding = torch.randn(rays.n_rays, 32, generator=gen)
    ys, xs = torch.arange(500, 524), torch.arange(900, 940)
    idx = (ys[:, None] * 1920 + xs[None, :]).reshape(-1)
    hdec = lp.DecoderParams(dec.mlp_params.to(dev), dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, 3)
    with torch.no_grad():
        out = lp.lightplane_renderer(rays.to(dev), [g.to(dev) for g in grids], hdec, num_samples=32, gain=1.0)
    o_out = O.lightplane_renderer_naive(rays[idx], grids, dec, num_samples=32, gain=1.0)
    for nm, a, b in zip(("ray_length", "neg_log_t", "feature"), out, o_out):
        _assert_close(f"1080p: {nm}", a[idx.to(dev)], b.detach().numpy())


_GOLDEN_CHILD = r"""
import sys
sys.path.insert(0, {root!r})
import pytest
sys.exit(pytest.main([{root!r} + "/tests/test_gpu_parity.py", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "-k",
                      "test_renderer_matches_oracle_and_golden and auto or cfg2_sized or early_termination"]))
"""


@pytest.mark.parametrize("env", [{"LP_BF3_NW": "8"}, {"LP_LOOP_NO_SHALLOW": "1"}, {"LP_LOOP": "1", "LP_SEG_FWD": "0"}],
                         ids=["bf3_backward_eight_wave_workgroups", "looped_deep_instantiations", "looped_eight_wave_forward"])
def test_golden_suite_on_the_other_kernel_families(env):
    """Kernels the default selection does not launch on these cases but a user can reach: the eight-wave-workgroup form of the
    tuned bf16x3 backward (what more than 64 beyond-far samples select; LP_BF3_NW=8 forces it) and the deep one-wave-per-SIMD
    instantiations of the layer-looped backward on the shallow decoders (LP_LOOP_NO_SHALLOW=1; by default those run the
    two-waves-per-SIMD instantiations of lp_renderer_loop_shallow.hip) and the eight-wave-workgroup forward of the two-block looped
    kernels (2/2/2 x 64 through LP_LOOP=1, with the small-batch segment-parallel forward off so that the march kernel runs).  The golden / cfg-2-sized / early-termination Renderer
    tests once more, so that every kernel that can be launched is held to the oracle.  (Until round 3 this test ran the
    fp32-MFMA generation of the Renderer kernels, retired in round 4.)"""
    r = subprocess.run([sys.executable, "-c", _GOLDEN_CHILD.format(root=ROOT)], cwd=ROOT, env=dict(os.environ, **env),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500)
    assert r.returncode == 0, r.stdout.decode()[-3000:]


_TM_CHILD = r"""
import sys
sys.path.insert(0, {root!r})
import pytest
sys.exit(pytest.main([{root!r} + "/tests/test_gpu_coherent.py", {root!r} + "/tests/test_gpu_config_scale.py", {root!r} + "/tests/test_gpu_parity.py",
                      "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "-k",
                      "triplane_s88 or voxel_b2_rgba_s96 or triplane_scaffold_noise_s70 or voxel_c32_s72 or test_flips_are_flips or cfg2_sized or c16_s128"]))
"""


def test_coherent_and_config_scale_cases_through_the_transposed_march():
    """LIGHTPLANE_AMD_MARCH_ORDER=samples sends every eligible launch (tuned family, >= 32 samples, no beyond-far samples) through the
    transposed march -- also the IMAGE-COHERENT ones the default would march rays per wavefront: a real 1080p launch, four of the
    segmented-backward cases (it replaces the segment-parallel march there), the cfg-2-sized properties and the proof cases, in a
    child process.  (The WHOLE GPU suite passes that way -- the headline launch with all 65 536 rays and its proof included -- but
    for two tests that assert the default's kernel name / setting: profiles/r06_transposed_march.txt, section 5.)"""
    r = subprocess.run([sys.executable, "-c", _TM_CHILD.format(root=ROOT)], cwd=ROOT, env=dict(os.environ, LIGHTPLANE_AMD_MARCH_ORDER="samples"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500)
    assert r.returncode == 0, r.stdout.decode()[-3000:]

"""The weight-gradient quadrant rounds of the tuned Renderer backward after their LDS operand reads were software-pipelined (round 9:
``dw_quadrant_bf_pipe``, lp_renderer_mfma_bwd.h -- the eight transposed reads of source wave v + 1 are issued before the products of
wave v).  Only the ORDER of instructions changed, so what can go wrong is a read that comes too early or from the wrong place: an
operand of the wrong source wave, a tile that is not published yet (the previous sample's or the previous layer's is still there), a
branch of ``want_params`` / ``gg`` that leaves a read without its store.  Everything goes through the public ``lightplane_renderer``
with ``kernel=LP_KERNEL_MFMA`` and the bars of tests/test_gpu_parity.py: the fp64 oracle with the kernel's own ReLU decisions forced
onto it through the DUMP twin, 1e-4 of the tensor's largest entry, no allowance.

* base grid: 160 rays (one full four-wave workgroup + a tail workgroup of one wave of rays and three waves of invalid lanes) and 96
  rays (the fourth wave of the workgroup is all invalid), a triplane of 8 x 8 cells with 16 and 32 channels, 3 and 4 colour channels,
  1 / 2 / 7 / 33 samples;
* wrong source wave: the upstream gradients of the four waves of a workgroup are scaled by 1, 2^8, 2^-8, 2^4 (exact in fp32) and every
  wave's rays carry another encoding scale, in the four rotations of that assignment.  A CPU test shows with the fp64 oracle alone that
  for every pair of waves one of the four cases moves some weight-gradient entry of every hidden layer by more than 100 bars when one
  wave's contribution stands in for the other's;
* stale tile: two and seven samples with a gain so large that the nearest sample is opaque -- the transmittance behind it underflows
  to exactly zero, in fp32 and in fp64 -- and no upstream gradient on -log T: the opacity gradient is exactly zero at EVERY sample and
  the colour gradient at every sample but the nearest (the last the far -> near sweep visits).  The whole opacity head's parameter
  gradient is exactly zero in the oracle and has to be exactly zero here: a dY tile of the colour layer's round still standing when
  the opacity layer's round reads, or anything non-zero read too early, shows;
* only the grid gradient, only the parameter gradient, only ``grad_encoding`` requested: each agrees with the all-leaves call (2e-5
  of its largest entry; outputs and ``grad_encoding`` bit for bit);
* one case each through the segmented instantiation, ``LP_ARITH_FP32`` (fp32 quadrants: the pipelined rounds are compiled out) and a
  32-channel voxel grid."""

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import Rays, _lib
from lightplane_amd.params import flatten_decoder_params, flattened_decoder_params_to_list
from tests.partial_grad_cases import NO_SEG, RendererEntry, config_set
from tests.synth import _rand_mlp, grid_sizes_for, random_grids, random_rays
from tests.test_gpu_coherent import oracle_renderer64
from tests.test_gpu_parity import (REL_TOL, _dev, _rel_err, forced_oracle_check, has_dump_twin, oracle_forced, run_hip_renderer,
                                   run_hip_renderer_with_dump)
from tests.test_gpu_partial_grads import _bit_identical, _close, _last_backward, run_renderer

gpu = pytest.mark.gpu

CELLS = 8
HID = 32
KERNEL = _lib.LP_KERNEL_MFMA
SHAPES = [(16, 3), (16, 4), (32, 3), (32, 4)]   # (grid channels, colour channels)
SHAPE_IDS = [f"c{c}_nc{n}" for c, n in SHAPES]
PARAM_STD = 0.1
WAVE = 32
GRAD_SCALES = (1.0, 2.0 ** 8, 2.0 ** -8, 2.0 ** 4)   # upstream gradients of the four waves of a workgroup (exact in fp32)
ENC_SCALES = (1.0, 0.25, 4.0, 2.0)                     # encoding scale of their rays
ROTATIONS = (0, 1, 2, 3)                               # wave w takes entry (w + rotation) % 4 of both: every wave is the loud one once
OPAQUE_GAIN = 1.0e5


def _decoder(gen, C, color_chn):
    wt, bt = _rand_mlp(gen, 2, C, HID, HID, PARAM_STD)
    wo, bo = _rand_mlp(gen, 2, HID, HID, 1, PARAM_STD)
    wc, bc = _rand_mlp(gen, 2, HID, HID, color_chn, PARAM_STD)
    flat, nt, no, nc = flatten_decoder_params(wt, bt, wo, bo, wc, bc, True)
    return lp.DecoderParams(flat, nt, no, nc, color_chn)


def _case(C, color_chn, num_samples, seed, n_rays=160, triplane=True, gain=1.0):
    gen = torch.Generator().manual_seed(seed)
    sizes = grid_sizes_for((1, CELLS, CELLS, CELLS, C), triplane)
    grids = random_grids(gen, sizes)
    dec = _decoder(gen, C, color_chn)
    rays = random_rays(gen, n_rays, 1, HID)
    cfg = dict(num_samples=num_samples, gain=gain, num_samples_inf=0, mask_out_of_bounds_samples=False, contract_coords=False,
               inject_noise_sigma=0.0, inject_noise_seed=0)
    up = (torch.randn(n_rays, generator=gen), torch.randn(n_rays, generator=gen), torch.randn(n_rays, color_chn, generator=gen))
    return dict(rays=rays, grids=grids, color_grids=None, decoder=dec, scaffold=None, cfg=cfg, sizes=sizes, upstream=up)


def _proof(name, d, dev):
    """forced_oracle_check on the tuned family's rays-per-wavefront backward, unsegmented -> (production results, forced oracle's)."""
    with config_set(**NO_SEG):
        assert lp.kernel_family(d["rays"], d["grids"], d["decoder"], kernel=KERNEL) == 1 and has_dump_twin(d, kernel=KERNEL, march_order="rays")
        _, prod, forced = forced_oracle_check(name, d, dev, kernel=KERNEL, march_order="rays", return_results=True)
    assert b"tuned family, rays per wavefront" in _last_backward(), _last_backward()
    return prod, forced


# ---- base grid ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("num_samples", [1, 2, 7, 33])
@pytest.mark.parametrize("C,color_chn", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("n_rays", [160, 96])
def test_base_grid(n_rays, C, color_chn, num_samples):
    dev = _dev()
    d = _case(C, color_chn, num_samples, seed=900 + C + color_chn + num_samples, n_rays=n_rays)
    prod, _ = _proof(f"operand-pipeline base R{n_rays} c{C} nc{color_chn} S{num_samples}", d, dev)
    assert float(prod[1].abs().max()) > 0.0


# ---- wrong source wave -------------------------------------------------------------------------------------------------------------
def _wave_case(C, rotation):
    """160 rays, seven samples; wave w of a workgroup (rays 32 w .. 32 w + 31 of every 128) has its upstream gradients scaled by
    GRAD_SCALES[(w + rotation) % 4] and its ray encodings by ENC_SCALES[(w + rotation) % 4]."""
    d = _case(C, 3, 7, seed=940 + C)
    wave = (torch.arange(160) // WAVE) % 4
    idx = (wave + rotation) % 4
    gs, es = torch.tensor(GRAD_SCALES)[idx], torch.tensor(ENC_SCALES)[idx]
    r = d["rays"]
    d["rays"] = Rays(directions=r.directions, origins=r.origins, grid_idx=r.grid_idx, near=r.near, far=r.far, encoding=r.encoding * es[:, None])
    g_len, g_nlt, g_feat = d["upstream"]
    d["upstream"] = (g_len * gs, g_nlt * gs, g_feat * gs[:, None])
    return d


def _hidden_weight_blocks(flat, dec):
    """the four hidden-layer weight gradients (trunk 1, trunk 2, opacity hidden, colour hidden) out of a flat parameter gradient"""
    ps = flattened_decoder_params_to_list(flat, dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color)
    return dict(t1=ps[0][0], t2=ps[0][1], o1=ps[2][0], c1=ps[4][0])


@pytest.mark.parametrize("C", [16, 32])
def test_wave_scales_tell_the_source_waves_apart(C):
    """CPU, fp64 oracle alone: the parameter gradient is linear in the upstream gradients, so the contribution of wave w of the full
    workgroup is the oracle's gradient over that wave's rays alone.  A quadrant round that takes the operands of
    wave a where wave b's belong moves the sum by (contribution of a) - (contribution of b): for every pair of waves and every hidden
    layer, in at least one of the cases the GPU test runs, that is more than 100 bars of the tensor the bar is taken of."""
    found = {}
    for rot in ROTATIONS:
        d = _wave_case(C, rot)
        parts = []   # the oracle over the rays of one wave at a time: waves 0..3 of the full workgroup, then the tail workgroup's wave
        for w in range(5):
            idx = torch.arange(WAVE * w, WAVE * (w + 1))
            dw = dict(d, rays=d["rays"][idx], upstream=tuple(u[idx] for u in d["upstream"]))
            parts.append(oracle_renderer64(dw)[1])
        bar = REL_TOL * float(sum(parts).abs().max())
        contrib = [_hidden_weight_blocks(p, d["decoder"]) for p in parts[:4]]
        for a in range(4):
            for b in range(a + 1, 4):
                for layer in ("t1", "t2", "o1", "c1"):
                    moved = float((contrib[a][layer] - contrib[b][layer]).abs().max()) / bar
                    found[(a, b, layer)] = max(found.get((a, b, layer), 0.0), moved)
    weakest = min(found, key=found.get)
    print(f"C = {C}: weakest (wave, wave, layer) {weakest}: {found[weakest]:.0f} bars")
    assert found[weakest] > 100.0, f"swapping the waves {weakest[:2]} in the round of layer {weakest[2]} moves no entry by more than {found[weakest]:.1f} bars"


@gpu
@pytest.mark.parametrize("rotation", ROTATIONS)
@pytest.mark.parametrize("C", [16, 32])
def test_every_wave_at_its_own_scale(C, rotation):
    dev = _dev()
    _proof(f"operand-pipeline wave scales c{C} rot{rotation}", _wave_case(C, rotation), dev)


# ---- stale tile --------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("num_samples", [2, 7])
@pytest.mark.parametrize("C,color_chn", [(16, 3), (32, 4)], ids=["c16_nc3", "c32_nc4"])
def test_gradient_on_one_sample_only(C, color_chn, num_samples):
    dev = _dev()
    d = _case(C, color_chn, num_samples, seed=960 + C + num_samples, gain=OPAQUE_GAIN)
    g_len, g_nlt, g_feat = d["upstream"]
    d["upstream"] = (g_len, torch.zeros_like(g_nlt), g_feat)
    name = f"operand-pipeline one sample c{C} nc{color_chn} S{num_samples}"
    prod, forced = _proof(name, d, dev)
    gp, f_gp = prod[1].cpu(), forced[1]
    zero = f_gp == 0
    dec = d["decoder"]
    f_blocks, z_blocks = _hidden_weight_blocks(f_gp, dec), _hidden_weight_blocks(zero, dec)
    assert bool(z_blocks["o1"].all()), "the opacity hidden layer has a gradient in the fp64 oracle: the case is not what it is meant to be"
    assert all(float(f_blocks[k].abs().max()) > 0.0 for k in ("t1", "t2", "c1")), "no colour gradient reaches the trunk"
    n = int((gp[zero] != 0).sum())
    print(f"{name}: {int(zero.sum())} of {zero.numel()} parameter-gradient entries exactly zero in the fp64 oracle, {n} of them not zero here")
    assert n == 0, f"{name}: {n} parameter-gradient entries the oracle leaves at exactly zero are not zero"


# ---- want_params / gg branches -----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("num_samples", [2, 33])
@pytest.mark.parametrize("C,color_chn", [(16, 3), (32, 4)], ids=["c16_nc3", "c32_nc4"])
def test_only_one_gradient_requested(C, color_chn, num_samples):
    dev = _dev()
    d = _case(C, color_chn, num_samples, seed=980 + C + num_samples)
    e = RendererEntry("operand_pipeline", "tuned four-wave full-batch kernel, plain march, triplane", None, kernel=KERNEL)
    base = run_renderer(e, d, dev, ("P", "E", "G"))
    assert b"tuned family, rays per wavefront" in _last_backward(), _last_backward()
    for subset in (("G",), ("P",), ("E",)):
        got = run_renderer(e, d, dev, subset)
        tag = f"operand-pipeline c{C} nc{color_chn} S{num_samples} [{'+'.join(subset)}]"
        for nm, a, b in zip(("ray_length", "neg_log_t", "feature"), got["out"], base["out"]):
            _bit_identical(f"{tag} {nm}", a, b)
        assert (got["P"] is not None) == ("P" in subset) and (got["E"] is not None) == ("E" in subset)
        assert all((g is not None) == ("G" in subset) for g in got["G"])
        if "P" in subset:
            _close(f"{tag} grad_mlp_params", got["P"], base["P"])
        if "E" in subset:
            _bit_identical(f"{tag} grad_encoding", got["E"], base["E"])
        if "G" in subset:
            for i, (a, b) in enumerate(zip(got["G"], base["G"])):
                _close(f"{tag} grad_grid{i}", a, b)


# ---- other instantiations ----------------------------------------------------------------------------------------------------------
@gpu
def test_segmented_instantiation():
    """The same 160 rays take the segment-parallel sweep by default: 21 samples = three LP_SEG_LEN blocks, the last one partial."""
    dev = _dev()
    d = _case(16, 3, 21, seed=1001)
    assert lp.backward_segments(d["rays"], d["grids"], d["decoder"], 21, 0, kernel=KERNEL, march_order="rays") > 1
    assert has_dump_twin(d, kernel=KERNEL, march_order="rays")
    forced_oracle_check("operand-pipeline segmented", d, dev, kernel=KERNEL, march_order="rays")
    assert b"tuned family, rays per wavefront" in _last_backward(), _last_backward()


@gpu
def test_fp32_arithmetic_instantiation():
    """LP_ARITH_FP32 has no DUMP twin; its recompute is the default instantiation's (three-limb products), so the ReLU decisions the
    default's twin reports are forced onto the fp64 oracle and the fp32-arithmetic launch is held to that."""
    dev = _dev()
    d = _case(16, 3, 7, seed=1002)
    with config_set(**NO_SEG):
        _, dump, wps = run_hip_renderer_with_dump(d, dev, KERNEL, march_order="rays")
        out, gp, ge, gg, _ = run_hip_renderer(d, dev, KERNEL, march_order="rays", arithmetic=_lib.LP_ARITH_FP32)
    assert b"tuned family, rays per wavefront" in _last_backward(), _last_backward()
    f_out, f_gp, f_ge, f_gg, _, _ = oracle_forced(d, dump, words_per_site=wps)
    worst = {nm: _rel_err(a, b.numpy()) for nm, a, b in
             [("ray_length", out[0], f_out[0]), ("neg_log_t", out[1], f_out[1]), ("feature", out[2], f_out[2]), ("grad_mlp_params", gp, f_gp),
              ("grad_encoding", ge, f_ge)] + [(f"grad_grid{i}", a, b) for i, (a, b) in enumerate(zip(gg, f_gg))]}
    print("operand-pipeline LP_ARITH_FP32: max err / scale: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= REL_TOL}
    assert not bad, f"LP_ARITH_FP32 against the forced fp64 oracle misses {REL_TOL:g}: {bad}"


@gpu
def test_voxel_grid_c32():
    dev = _dev()
    d = _case(32, 3, 7, seed=1003, triplane=False)
    _proof("operand-pipeline voxel c32", d, dev)

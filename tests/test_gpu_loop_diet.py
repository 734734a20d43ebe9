"""The sample loop of the tuned Renderer backward after its bookkeeping diet (round 8): every rewritten piece, pinned through the
public ``lightplane_renderer`` with ``kernel=LP_KERNEL_MFMA`` and the suite's own bars (tests/test_gpu_parity.py: fp64 oracle with the
kernel's own ReLU decisions forced onto it through the DUMP twin, 1e-4 of the tensor's largest entry, no allowance).

What changed in the kernel and what holds it here:
* the ReLU gates of the head layers (d ho through a shifted bit mask, ``mask_push`` / ``mask_gate``; d hc keeps ``mask_bit`` /
  ``mask_apply`` -- reading it back from the LDS tile of hc was tried and lost on the clock): colour-head biases that open every gate, close every gate (gradient of W_c1 and b_c1 EXACTLY zero) and open every
  other one -- and the DUMP twin's c1 word has to say exactly that for every visited sample;
* grid taps: validity folded into the per-axis weights, indices clamped into the plane (gather) / into [0, size - 2] (scatter): rays
  that leave the cube through each of its six faces, so that taps straddle every border of every plane, and rays that never enter it;
  next to the oracle bar every texel the fp64 oracle leaves at exactly zero has to be exactly zero -- an invalid tap adds nothing
  anywhere, row 0 included;
* the transmittance in front of a sample is carried from the sample behind it and recomputed only where a checkpoint of -log T is
  reloaded: 33 samples put the reload inside the march (LP_NLT_CKPT = 32);
* the limb-tile stores sit in the ``want_params`` branches, the gather / scatter in the ``gg`` ones: the same call with only the grid
  gradient and only the parameter gradient requested agrees with the all-leaves call (2e-5 of its largest entry: the same kernel, the
  atomics in another order; the outputs bit for bit).

Shapes: 160 rays (one full four-wave workgroup + a tail workgroup of one wave of rays and three waves of invalid lanes), a triplane of
8 x 8 cells with 16 and with 32 channels, 3 and 4 colour channels, 1 / 7 / 33 samples."""
import math

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import Rays, _lib
from lightplane_amd.params import flatten_decoder_params, flattened_decoder_params_to_list
from lightplane_amd.renderer import relu_dump_recorder
from tests.partial_grad_cases import NO_SEG, RendererEntry, config_set
from tests.synth import _rand_mlp, grid_sizes_for, random_grids, random_rays
from tests.test_gpu_parity import _dev, forced_oracle_check, has_dump_twin, run_hip_renderer
from tests.test_gpu_partial_grads import _bit_identical, _close, _last_backward, run_renderer

pytestmark = pytest.mark.gpu

N_RAYS = 160
CELLS = 8
HID = 32
KERNEL = _lib.LP_KERNEL_MFMA
SHAPES = [(16, 3), (16, 4), (32, 3), (32, 4)]   # (grid channels, colour channels)
BIAS = 4.0   # |b_c1| of the scripted gates: the rest of the pre-activation is N(0, ~0.6^2) with PARAM_STD = 0.1 (7 sigma)
PARAM_STD = 0.1


def _decoder(gen, C, color_chn, gates=None):
    """2/2/2 x 32 decoder (the tuned shape), N(0, PARAM_STD) parameters; ``gates``: b_c1 = +BIAS (open) / -BIAS (closed) per unit."""
    wt, bt = _rand_mlp(gen, 2, C, HID, HID, PARAM_STD)
    wo, bo = _rand_mlp(gen, 2, HID, HID, 1, PARAM_STD)
    wc, bc = _rand_mlp(gen, 2, HID, HID, color_chn, PARAM_STD)
    if gates is not None:
        bc[0] = torch.where(gates, torch.tensor(BIAS), torch.tensor(-BIAS))
    flat, nt, no, nc = flatten_decoder_params(wt, bt, wo, bo, wc, bc, True)
    return lp.DecoderParams(flat, nt, no, nc, color_chn)


def _face_rays(gen, enc_dim):
    """120 rays that leave the cube [-1, 1]^3 through each of its six faces (20 per face: the march runs from 0.8 inside to 1.3
    outside along the face's axis, anywhere in [-1.2, 1.2] along the other two -- so corners and edges are crossed as well) and 40
    rays that never enter it.  Sample points are origin + t * direction, t in [0, 1]."""
    p0, p1 = [], []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            a = torch.rand(20, 3, generator=gen) * 2.4 - 1.2
            b = torch.rand(20, 3, generator=gen) * 2.4 - 1.2
            a[:, axis], b[:, axis] = sign * 0.8, sign * 1.3
            p0.append(a)
            p1.append(b)
    for axis in range(2):   # entirely outside: beyond +x, beyond -y
        a = torch.rand(20, 3, generator=gen) * 3.0 - 1.5
        b = torch.rand(20, 3, generator=gen) * 3.0 - 1.5
        a[:, axis], b[:, axis] = (1.1, 1.6) if axis == 0 else (-1.6, -1.1)
        p0.append(a)
        p1.append(b)
    p0, p1 = torch.cat(p0), torch.cat(p1)
    perm = torch.randperm(N_RAYS, generator=gen)   # (neighbouring lanes in different situations: run merges of every kind)
    p0, p1 = p0[perm], p1[perm]
    return Rays(directions=(p1 - p0).contiguous(), origins=p0.contiguous(), grid_idx=torch.zeros(N_RAYS, dtype=torch.long),
                near=torch.zeros(N_RAYS), far=torch.ones(N_RAYS), encoding=torch.randn(N_RAYS, enc_dim, generator=gen))


def _case(C, color_chn, num_samples, seed, gates=None, face_rays=False, mask_oob=False):
    gen = torch.Generator().manual_seed(seed)
    sizes = grid_sizes_for((1, CELLS, CELLS, CELLS, C), True)
    grids = random_grids(gen, sizes)
    dec = _decoder(gen, C, color_chn, gates)
    rays = _face_rays(gen, HID) if face_rays else random_rays(gen, N_RAYS, 1, HID)
    cfg = dict(num_samples=num_samples, gain=1.0, num_samples_inf=0, mask_out_of_bounds_samples=mask_oob, contract_coords=False,
               inject_noise_sigma=0.0, inject_noise_seed=0)
    up = (torch.randn(N_RAYS, generator=gen), torch.randn(N_RAYS, generator=gen), torch.randn(N_RAYS, color_chn, generator=gen))
    return dict(rays=rays, grids=grids, color_grids=None, decoder=dec, scaffold=None, cfg=cfg, sizes=sizes, upstream=up)


def _proof(name, d, dev):
    """forced_oracle_check on the tuned family's rays-per-wavefront backward, unsegmented; returns (production results, forced fp64
    oracle's results)."""
    with config_set(**NO_SEG):
        assert lp.kernel_family(d["rays"], d["grids"], d["decoder"], kernel=KERNEL) == 1 and has_dump_twin(d, kernel=KERNEL, march_order="rays")
        # (march_order: a batch this small with 32 samples or more would take the transposed march by default)
        _, prod, forced = forced_oracle_check(name, d, dev, kernel=KERNEL, march_order="rays", return_results=True)
    assert b"tuned family, rays per wavefront" in _last_backward(), _last_backward()
    return prod, forced


def _untouched_texels_stay_zero(name, prod, forced):
    for i, (g, f) in enumerate(zip(prod[3], forced[3])):
        zero = (f == 0).to(g.device)
        n = int((g[zero] != 0).sum())
        print(f"{name}: grad_grid{i}: {int(zero.sum())} of {zero.numel()} entries exactly zero in the fp64 oracle, {n} of them not zero here")
        assert n == 0, f"{name}: grad_grid{i} has {n} non-zero entries where no valid tap of any ray lands"


GATES = {"open": torch.ones(HID, dtype=torch.bool), "closed": torch.zeros(HID, dtype=torch.bool),
         "alternating": torch.arange(HID) % 2 == 0}


@pytest.mark.parametrize("gate", list(GATES))
@pytest.mark.parametrize("C,color_chn", SHAPES, ids=[f"c{c}_nc{n}" for c, n in SHAPES])
def test_colour_gates(C, color_chn, gate):
    dev = _dev()
    d = _case(C, color_chn, 7, seed=800 + C + color_chn, gates=GATES[gate])
    name = f"loop-diet gates {gate} c{C} nc{color_chn}"
    prod, forced = _proof(name, d, dev)
    # the DUMP twin reports exactly the scripted decisions of the colour hidden layer, for every sample it visited
    with config_set(**NO_SEG), relu_dump_recorder() as rec:
        run_hip_renderer(d, dev, KERNEL, march_order="rays")
    dump = rec.dump.cpu().to(torch.int64) & 0xFFFFFFFF
    assert dump.shape == (N_RAYS, 7, 5) and bool((dump[..., 4] == 1).all()), "every sample of a plain march contributes"
    want = int(sum(1 << f for f in range(HID) if bool(GATES[gate][f])))
    wrong = int((dump[..., 3] != want).sum())
    assert wrong == 0, f"{name}: {wrong} of {N_RAYS * 7} samples report other c1 decisions than {want:#010x}"
    gw = flattened_decoder_params_to_list(prod[1].cpu(), *(d["decoder"].n_hidden_trunk, d["decoder"].n_hidden_opacity, d["decoder"].n_hidden_color))
    g_wc1, g_bc1 = gw[4][0], gw[5][0]   # [in, out], [out]
    closed = ~GATES[gate]
    assert float(g_wc1[:, closed].abs().max() if closed.any() else 0.0) == 0.0 and float(g_bc1[closed].abs().max() if closed.any() else 0.0) == 0.0, \
        f"{name}: a closed unit of the colour hidden layer has a gradient"
    if gate != "closed":
        assert float(g_wc1[:, ~closed].abs().max(dim=0).values.min()) > 0.0, f"{name}: an open unit of the colour hidden layer has no gradient"
    else:
        assert float(prod[2].abs().max()) == 0.0, f"{name}: the ray encoding reaches the outputs through closed gates only"
    _untouched_texels_stay_zero(name, prod, forced)


@pytest.mark.parametrize("mask_oob", [False, True], ids=["keep_oob", "mask_oob"])
@pytest.mark.parametrize("num_samples", [1, 7])
@pytest.mark.parametrize("C,color_chn", [(16, 3), (32, 4)], ids=["c16_nc3", "c32_nc4"])
def test_taps_across_every_border(C, color_chn, num_samples, mask_oob):
    dev = _dev()
    d = _case(C, color_chn, num_samples, seed=830 + C + num_samples, face_rays=True, mask_oob=mask_oob)
    name = f"loop-diet borders c{C} nc{color_chn} S{num_samples} {'mask' if mask_oob else 'keep'}"
    prod, forced = _proof(name, d, dev)
    if num_samples > 1:
        assert all(float(g.abs().max()) > 0 for g in prod[3]), "no ray reached the planes: the comparison is between zeros"
    _untouched_texels_stay_zero(name, prod, forced)


@pytest.mark.parametrize("C,color_chn", SHAPES, ids=[f"c{c}_nc{n}" for c, n in SHAPES])
def test_checkpoint_reload_inside_the_march(C, color_chn):
    """33 samples: the far -> near sweep starts from the checkpoint behind sample 32 and reloads the one behind sample 31 -- the
    carried transmittance has to be recomputed there and nowhere else.  (The rays are about 3 long and softplus(0) = 0.69: the
    transmittance falls to about e^-2 along a ray, so the carried value matters at every sample.)"""
    dev = _dev()
    assert 1 < math.ceil(33 / _lib.LP_NLT_CKPT) and (33 - 1) % _lib.LP_NLT_CKPT == 0, "the shape no longer puts a reload inside the march"
    d = _case(C, color_chn, 33, seed=860 + C + color_chn)
    name = f"loop-diet checkpoints c{C} nc{color_chn}"
    prod, forced = _proof(name, d, dev)
    t = torch.exp(-prod[0][1].detach().cpu())
    assert 0.02 < float(t.median()) < 0.98, f"median transmittance {float(t.median()):.3f}: the compositing is not exercised"
    _untouched_texels_stay_zero(name, prod, forced)


@pytest.mark.parametrize("num_samples", [1, 7, 33])
@pytest.mark.parametrize("C,color_chn", [(16, 4), (32, 3)], ids=["c16_nc4", "c32_nc3"])
def test_only_some_gradients_requested(C, color_chn, num_samples):
    dev = _dev()
    d = _case(C, color_chn, num_samples, seed=890 + C + num_samples, face_rays=(num_samples == 7))
    e = RendererEntry("loop_diet", "tuned four-wave full-batch kernel, plain march, triplane", None, kernel=KERNEL)
    base = run_renderer(e, d, dev, ("P", "E", "G"))
    assert b"tuned family, rays per wavefront" in _last_backward(), _last_backward()
    for subset in (("G",), ("P",), ("E", "G"), ("P", "E")):
        got = run_renderer(e, d, dev, subset)
        tag = f"loop-diet c{C} nc{color_chn} S{num_samples} [{'+'.join(subset)}]"
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
                if float(b.abs().max()) == 0.0:   # (one sample at the ray's near end may reach no plane at all)
                    assert float(a.abs().max()) == 0.0
                else:
                    _close(f"{tag} grad_grid{i}", a, b)

"""Case table and fp64 definition of ``lightplane_amd.kplanes_render_samples`` (tests/test_kplanes_render_host.py checks them without
a GPU, tests/test_gpu_kplanes_render.py holds the kernels to them).

Definition: ``tests.test_gpu_kplanes.reference`` at ``depths * direction + origin`` in fp64 on the fp32 inputs, the decoder from the
oracle's pieces under ``relu_margin_recorder`` as tests/kplanes_points_cases.py composes them, then
``tests.compositing_cases.composite``; autograd gives the gradients; upstream gradients are random on all four results.  A sample near
a tie of the fp64 reference (the conditions of kplanes_points_cases: ReLU margin, a plane or time coordinate near an integer on any
scale, the contraction's kink, a cube face with mask or scaffold, a scaffold cell boundary) gets ``delta = 0`` in the inputs of
reference AND kernel (at most ``MAX_ZEROED`` of a case): it neither contributes nor receives anything.  A seed that misses the cap is
changed, never the bar."""
import dataclasses

import torch

import lightplane_amd as lp
from oracle import lightplane_oracle as O
from tests import compositing_cases as CC
from tests import importance_cases as IC
from tests import render_samples_cases as RC
from tests import test_gpu_kplanes as KP
from tests.points_cases import CELL_EPS, MAX_ZEROED, RELU_MARGIN, TOL, _near_half, _unnorm  # noqa: F401
from tests.synth import random_decoder, random_rays

DYN = KP.DYN   # n = (5, 9), m = (4, 4), C = 8
#   name: layout, (trunk, opacity, colour layers, hidden), (R, S), batch, depths, mask, contract, scaffold shape, gain (None: median
#   -log T 800), times per sample
CASES = {
    "dynamic_222x32": (DYN, (2, 2, 2, 32), (9, 65), 2, "uniform", False, False, None, 1.7, False),
    "static_112x32": (dict(DYN, time_resolution=None), (1, 1, 2, 32), (3, 64), 2, "uniform", False, False, None, 1.7, False),
    "c4_112x32": (dict(DYN, channels=4), (1, 1, 2, 32), (3, 63), 2, "uniform", False, False, None, 1.7, False),
    "c64_112x64": (dict(DYN, time_resolution=4, channels=64), (1, 1, 2, 64), (3, 63), 2, "uniform", False, False, None, 1.7, False),
    "notrunk_022x32": (dict(resolutions=(4, 8, 16, 32), time_resolution=6, channels=8), (0, 2, 2, 32), (3, 130), 2, "resampled", False,
                       False, None, 1.7, False),
    "point_times": (DYN, (1, 1, 2, 32), (3, 65), 2, "uniform", False, False, None, 1.7, True),
    "zeros": (DYN, (1, 1, 2, 32), (3, 65), 2, "uniform", False, False, None, 1.7, False),
    "contract_mask_scaffold": (DYN, (2, 2, 2, 32), (9, 130), 1, "beyond_far", True, True, (1, 5, 4, 6), 1.7, False),
    "opaque": (DYN, (2, 2, 2, 32), (9, 200), 2, "uniform", False, False, None, None, False),
    "one_sample": (DYN, (2, 2, 2, 32), (1, 1), 2, "uniform", False, False, None, 1.7, False),
    "many_rays": (dict(resolutions=(8,), time_resolution=None, channels=4), (1, 1, 1, 8), (4099, 3), 2, "uniform", False, False, None,
                  1.7, False),
}
SEEDS = {name: 1500 + i for i, name in enumerate(CASES)}
ALL = list(CASES)
_INPUTS, _CACHE = {}, {}


def inputs(name):
    """the fp32 tensors of a case but its samples: rays (with encoding), times, planes, decoder, scaffold, the four upstream gradients"""
    if name not in _INPUTS:
        kw, (n_t, n_o, n_c, hidden), (R, S), B, depth, mask, contract, sc_shape, gain, per_sample = CASES[name]
        lay = lp.kplanes_layout(**kw)
        gen = torch.Generator().manual_seed(SEEDS[name])
        dec = random_decoder(gen, n_t, n_o, n_c, lay.out_channels, hidden, 3, std=(2.0 / hidden) ** 0.5)
        rays = random_rays(gen, R, B, int(dec.n_hidden_color[0]))
        if name == "dynamic_222x32":   # batch elements out of range: clamped
            rays = dataclasses.replace(rays, grid_idx=torch.tensor([0, 1, 1, 0, 5, -2, 1, 0, 1]))
        times = None
        if lay.n_planes == 6:          # beyond +-1: clamped
            times = (torch.rand((R, S) if per_sample else (R,), generator=gen) * 2 - 1) * 1.2
        shape = (B, lay.rows, lay.channels)   # magnitudes in [0.5, 1.5], one sign per (scene, channel): a product of six stays in range
        planes = (0.5 + torch.rand(shape, generator=gen)) * (torch.randint(0, 2, (B, 1, lay.channels), generator=gen) * 2 - 1)
        if name == "zeros":            # a third of the entries exactly 0, and every row of the xy plane of scale 0
            planes[torch.rand(shape, generator=gen) < 1 / 3] = 0.0
            planes[:, lay.offsets[0][0]:lay.offsets[0][1]] = 0.0
        scaffold = None if sc_shape is None else (torch.rand(sc_shape, generator=gen) < 0.6).float()
        ups = [torch.randn(R, generator=gen), torch.randn(R, generator=gen), torch.randn(R, 3, generator=gen), torch.randn(R, S, generator=gen)]
        _INPUTS[name] = dict(name=name, lay=lay, dec=dec, rays=rays, times=times, planes=planes, scaffold=scaffold, ups=ups, B=B,
                             depth=depth, mask=mask, contract=contract, gain=gain, R=R, S=S)
    return _INPUTS[name]


def host_samples(name):
    """fp32 (depths, deltas) of the case's regime from the definitions of the sample ops (the GPU test takes them from the ops)"""
    c = inputs(name)
    a, b = RC.split_samples(c["S"], c["depth"])
    if c["depth"] == "resampled":
        coarse = CC.placement(c["rays"], a, 0, RC.DISPARITY, torch.float32)[1]
        return IC.resample(c["rays"].origins, c["rays"].directions, RC.peaked_depths(coarse), RC.peaked_weights(c["R"], a), b,
                           dtype=torch.float32)[1:]
    return CC.placement(c["rays"], a, b, RC.DISPARITY, torch.float32)[1:]


def field(c, points, leaves, touched=None):
    """(opacity at gain 1, colour, ReLU margin) of the fp64 field at ``points [R, S, 3]``; ``touched [B, rows]``: rows a sample reads"""
    dec, gidx = c["dec"], c["rays"].grid_idx
    t64 = None if c["times"] is None else c["times"].double()
    (wt, bt), (wo, bo), (wc, bc) = O.split_decoder(leaves["params"], dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color)
    with O.relu_margin_recorder() as rec:
        feat = KP.reference(points, t64, leaves["planes"], gidx, c["lay"], c["mask"], c["contract"], touched)
        trunk = O._relu(O.mlp_forward(feat, wt, bt))
        raw = O.mlp_forward(trunk, wo, bo)[..., 0]
        craw = O.mlp_forward(trunk + leaves["enc"][:, None], wc, bc)[..., :3]
    occ = torch.ones_like(raw)
    if c["scaffold"] is not None:
        q = KP._contract(points.detach()) if c["contract"] else points.detach()
        occ = O.sample_scaffold_nearest(c["scaffold"].double(), q, gidx.clamp(0, c["B"] - 1))
    return torch.nn.functional.softplus(raw) * occ, torch.sigmoid(craw) * occ[..., None], rec.margin


def near_tie(c, p64, margin):
    """[R, S] bool: the samples the module docstring zeroes"""
    lay = c["lay"]
    q64 = KP._contract(p64) if c["contract"] else p64
    z = margin < RELU_MARGIN
    if c["scaffold"] is not None:
        sh = c["scaffold"].shape
        for ax, size in ((0, sh[3]), (1, sh[2]), (2, sh[1])):
            z = z | _near_half(_unnorm(q64[..., ax], size), CELL_EPS)
    if c["mask"] or c["scaffold"] is not None:
        z = z | ((q64.abs() - 1.0).abs() < KP.FACE_EPS).any(-1)
    if c["contract"]:
        a = p64.abs().sort(dim=-1, descending=True).values
        z = z | ((a[..., 0] - 1.0).abs() < KP.KINK_EPS) | ((a[..., 0] > 1.0) & ((a[..., 0] - a[..., 1]) < KP.KINK_EPS))
    t64 = None if c["times"] is None else c["times"].double()
    for s in range(lay.n_scales):
        for x, n in zip(KP._coords(q64, t64), [lay.spatial[s]] * 3 + ([lay.temporal[s]] if lay.temporal else [])):
            x = ((x + 1) / 2 * (n - 1)).clamp(-0.5, n - 0.5)   # (a coordinate clamped away has no kink)
            z = z | ((x - x.round()).abs() < KP.INT_EPS)
    return z


def case(name, depths, deltas, tag="host"):
    """the inputs of ``inputs(name)`` with fp32 ``deltas`` (near ties zeroed), ``gain``, the fp64 results ``out`` and gradients ``grads``
    at these fp32 samples; built once per (name, tag), never modified"""
    if (name, tag) in _CACHE:
        return _CACHE[(name, tag)]
    c = dict(inputs(name))
    d64 = depths.double()
    leaves = dict(planes=c["planes"].double().requires_grad_(True), params=c["dec"].mlp_params.double().requires_grad_(True),
                  enc=c["rays"].encoding.double().requires_grad_(True))
    touched = torch.zeros(c["B"], c["lay"].rows, dtype=torch.bool)
    p64 = d64[..., None] * c["rays"].directions.double()[:, None] + c["rays"].origins.double()[:, None]
    op1, col, margin = field(c, p64, leaves, touched)
    zeroed = near_tie(c, p64, margin)
    deltas = torch.where(zeroed, torch.zeros_like(deltas), deltas)
    if c["gain"] is None:
        c["gain"] = 800.0 / float((op1.detach() * deltas.double()).sum(-1).median())
    out = CC.composite(c["gain"] * op1, col, d64, deltas.double())
    sum((o * u.double()).sum() for o, u in zip(out, c["ups"])).backward()
    c.update(depths=depths, deltas=deltas, zeroed=zeroed, out=tuple(o.detach() for o in out), grads={k: v.grad for k, v in leaves.items()},
             untouched=~touched)
    _CACHE[(name, tag)] = c
    return c

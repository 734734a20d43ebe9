"""Case table and fp64 definition of ``lightplane_amd.hash_grid_render_samples`` (tests/test_hash_render_host.py checks them without a
GPU, tests/test_gpu_hash_render.py holds the kernels to them).

Definition: ``tests.test_gpu_hash_grid.reference`` at ``depths * direction + origin`` in fp64 on the fp32 inputs, the decoder from the
oracle's pieces as tests/hash_points_cases.py composes them, then ``tests.compositing_cases.composite``; autograd gives the gradients;
upstream gradients are random on all four results.  A sample near a tie of the fp64 reference (the conditions of hash_points_cases:
ReLU margin, level coordinate near an integer, contraction kink, cube face with mask or scaffold, scaffold cell boundary) gets
``delta = 0`` in the inputs of reference AND kernel (at most ``MAX_ZEROED`` of a case): it neither contributes nor receives anything.
A seed that misses the cap is changed, never the bar."""
import dataclasses

import torch

import lightplane_amd as lp
from oracle import lightplane_oracle as O
from tests import compositing_cases as CC
from tests import importance_cases as IC
from tests import render_samples_cases as RC
from tests import test_gpu_hash_grid as HG
from tests.hash_points_cases import MIXED
from tests.points_cases import CELL_EPS, MAX_ZEROED, RELU_MARGIN, TOL, _near_half, _unnorm  # noqa: F401
from tests.synth import random_decoder, random_rays

NGP = dict(n_levels=16, features_per_level=2, log2_table_size=10, base_resolution=16, finest_resolution=256)
#   name: layout, (trunk, opacity, colour layers, hidden), (R, S), batch, depths, mask, contract, scaffold shape, gain (None: median -log T 800)
CASES = {
    "mixed_222x32": (MIXED, (2, 2, 2, 32), (9, 65), 2, "uniform", False, False, None, 1.7),
    "f1_112x32": (dict(MIXED, features_per_level=1), (1, 1, 2, 32), (3, 64), 2, "uniform", False, False, None, 1.7),
    "f8_112x64": (dict(MIXED, features_per_level=8), (1, 1, 2, 64), (3, 63), 2, "uniform", False, False, None, 1.7),
    "ngp_022x32": (NGP, (0, 2, 2, 32), (3, 130), 2, "resampled", False, False, None, 1.7),
    "contract_mask_scaffold": (MIXED, (2, 2, 2, 32), (9, 130), 1, "beyond_far", True, True, (1, 5, 4, 6), 1.7),
    "opaque": (MIXED, (2, 2, 2, 32), (9, 200), 2, "uniform", False, False, None, None),
    "one_sample": (MIXED, (2, 2, 2, 32), (1, 1), 2, "uniform", False, False, None, 1.7),
    "many_rays": (dict(n_levels=2, features_per_level=1, log2_table_size=8, base_resolution=8, finest_resolution=32), (1, 1, 1, 8),
                  (4099, 3), 2, "uniform", False, False, None, 1.7),
}
SEEDS = {name: 1400 + i for i, name in enumerate(CASES)}
ALL = list(CASES)
_INPUTS, _CACHE = {}, {}


def inputs(name):
    """the fp32 tensors of a case but its samples: rays (with encoding), table, decoder, scaffold, the four upstream gradients"""
    if name not in _INPUTS:
        kw, (n_t, n_o, n_c, hidden), (R, S), B, depth, mask, contract, sc_shape, gain = CASES[name]
        lay = lp.hash_grid_layout(**kw)
        gen = torch.Generator().manual_seed(SEEDS[name])
        dec = random_decoder(gen, n_t, n_o, n_c, lay.channels, hidden, 3, std=(2.0 / hidden) ** 0.5)
        rays = random_rays(gen, R, B, int(dec.n_hidden_color[0]))
        if name == "mixed_222x32":   # batch elements out of range: clamped
            rays = dataclasses.replace(rays, grid_idx=torch.tensor([0, 1, 1, 0, 5, -2, 1, 0, 1]))
        table = torch.randn(B, lay.entries, lay.features_per_level, generator=gen)
        scaffold = None if sc_shape is None else (torch.rand(sc_shape, generator=gen) < 0.6).float()
        ups = [torch.randn(R, generator=gen), torch.randn(R, generator=gen), torch.randn(R, 3, generator=gen), torch.randn(R, S, generator=gen)]
        _INPUTS[name] = dict(name=name, lay=lay, dec=dec, rays=rays, table=table, scaffold=scaffold, ups=ups, B=B, depth=depth, mask=mask,
                             contract=contract, gain=gain, R=R, S=S)
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


def field(c, points, leaves):
    """(opacity at gain 1, colour, ReLU margin, features) of the fp64 field at ``points [R, S, 3]``"""
    dec, gidx = c["dec"], c["rays"].grid_idx
    (wt, bt), (wo, bo), (wc, bc) = O.split_decoder(leaves["params"], dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color)
    with O.relu_margin_recorder() as rec:
        feat = HG.reference(points, leaves["table"], gidx, c["lay"], c["mask"], c["contract"])
        trunk = O._relu(O.mlp_forward(feat, wt, bt))
        raw = O.mlp_forward(trunk, wo, bo)[..., 0]
        craw = O.mlp_forward(trunk + leaves["enc"][:, None], wc, bc)[..., :3]
    occ = torch.ones_like(raw)
    if c["scaffold"] is not None:
        q = HG._contract(points.detach()) if c["contract"] else points.detach()
        occ = O.sample_scaffold_nearest(c["scaffold"].double(), q, gidx.clamp(0, c["B"] - 1))
    return torch.nn.functional.softplus(raw) * occ, torch.sigmoid(craw) * occ[..., None], rec.margin, feat


def points_of(c, depths):
    return depths[..., None] * c["rays"].directions.double()[:, None] + c["rays"].origins.double()[:, None]


def near_tie(c, p64, margin):
    """[R, S] bool: the samples the module docstring zeroes"""
    q64 = HG._contract(p64) if c["contract"] else p64
    z = margin < RELU_MARGIN
    if c["scaffold"] is not None:
        sh = c["scaffold"].shape
        for ax, size in ((0, sh[3]), (1, sh[2]), (2, sh[1])):
            z = z | _near_half(_unnorm(q64[..., ax], size), CELL_EPS)
    if c["mask"] or c["scaffold"] is not None:
        z = z | ((q64.abs() - 1.0).abs() < HG.FACE_EPS).any(-1)
    if c["contract"]:
        a = p64.abs().sort(dim=-1, descending=True).values
        z = z | ((a[..., 0] - 1.0).abs() < HG.KINK_EPS) | ((a[..., 0] > 1.0) & ((a[..., 0] - a[..., 1]) < HG.KINK_EPS))
    for n_l in c["lay"].resolutions:
        x = ((q64 + 1) / 2 * n_l).clamp(-0.5, n_l + 0.5)   # (a coordinate clamped away has no kink)
        z = z | ((x - x.round()).abs() < HG.INT_EPS).any(-1)
    return z


def case(name, depths, deltas, tag="host"):
    """the inputs of ``inputs(name)`` with fp32 ``deltas`` (near ties zeroed), ``gain``, the fp64 results ``out`` and gradients ``grads``
    at these fp32 samples; built once per (name, tag), never modified"""
    if (name, tag) in _CACHE:
        return _CACHE[(name, tag)]
    c = dict(inputs(name))
    d64 = depths.double()
    leaves = dict(table=c["table"].double().requires_grad_(True), params=c["dec"].mlp_params.double().requires_grad_(True),
                  enc=c["rays"].encoding.double().requires_grad_(True))
    op1, col, margin, feat = field(c, points_of(c, d64), leaves)
    zeroed = near_tie(c, points_of(c, d64), margin)
    deltas = torch.where(zeroed, torch.zeros_like(deltas), deltas)
    if c["gain"] is None:
        c["gain"] = 800.0 / float((op1.detach() * deltas.double()).sum(-1).median())
    (touched,) = torch.autograd.grad(feat, leaves["table"], torch.ones_like(feat), retain_graph=True)   # (the weights are >= 0)
    out = CC.composite(c["gain"] * op1, col, d64, deltas.double())
    sum((o * u.double()).sum() for o, u in zip(out, c["ups"])).backward()
    c.update(depths=depths, deltas=deltas, zeroed=zeroed, out=tuple(o.detach() for o in out), grads={k: v.grad for k, v in leaves.items()},
             untouched=touched == 0)
    _CACHE[(name, tag)] = c
    return c

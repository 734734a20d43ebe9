"""Inputs and fp64 reference of the plane-field scaffold (tests/test_kplanes_scaffold_host.py holds the thresholds' gaps without a GPU,
tests/test_gpu_kplanes_scaffold.py holds the kernel to the reference).  Every case is built once per process and never modified.

Reference: ``tests.test_gpu_kplanes.reference`` in fp64 on the explicit lattice (one scalar time per call), the decoder from the
oracle's own pieces, ``gain * softplus``, the maximum over the timestamps; the occupancy threshold is
``tests.test_gpu_scaffold.unambiguous_threshold`` of that lattice.  A seed that misses the gap is changed, never the bar."""
import torch

import lightplane_amd as lp
from oracle import lightplane_oracle as O
from tests import test_gpu_kplanes as KP
from tests.synth import random_decoder
from tests.test_gpu_scaffold import _lattice, unambiguous_threshold

GAIN = 1.7
#   name: layout, (trunk, opacity layers, hidden), scaffold [B, D, H, W], times, dilate
CASES = {
    # two workgroups per row with a part-filled second; lattice finer than every plane; a clamped time; batch > 1
    "dyn_22x32_w70": (KP.DYN, (2, 2, 32), (2, 3, 4, 70), (-0.35, 1.2, 0.6), 1),
    # no time loop; W < 64
    "static_11x32": (dict(KP.DYN, time_resolution=None), (1, 1, 32), (1, 5, 4, 6), None, 0),
    # S C = 128: the widest tiles, the static product formed again per timestamp; a window wider than D and H
    "c64_11x64_w65": (dict(KP.DYN, time_resolution=4, channels=64), (1, 1, 64), (1, 2, 3, 65), (0.8, -0.45), 3),
    # four scales; no trunk; a one-point lattice (lin01 with n = 1)
    "notrunk_02x32_point": (dict(resolutions=(4, 8, 16, 32), time_resolution=6, channels=4), (0, 2, 32), (2, 1, 1, 1), (0.3,), 1),
    # a lattice far coarser than the plane: neighbouring lanes eight rows apart
    "coarse_11x32": (dict(resolutions=(33,), time_resolution=3, channels=8), (1, 1, 32), (1, 2, 2, 4), (-0.7, 0.15), 0),
}
SEEDS = {name: 1700 + i for i, name in enumerate(CASES)}
ALL = list(CASES)
_CACHE = {}


def oracle_opacity(planes, lay, dec, size, times, gain):
    """fp64 ``[B, D, H, W]``: the maximum over ``times`` (a list of floats, or None) of the decoder's opacity on the lattice"""
    B, D, H, W = size
    pts = _lattice(D, H, W).double().expand(B, -1, -1)
    (wt, bt), (wo, bo), _ = O.split_decoder(dec.mlp_params.double(), dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color)
    best = None
    for t in [None] if times is None else times:
        t64 = None if t is None else torch.full((B,), t, dtype=torch.float32).double()   # (the fp32 value the kernel reads)
        feat = KP.reference(pts, t64, planes.double(), torch.arange(B), lay, False, False)
        raw = O.mlp_forward(O._relu(O.mlp_forward(feat, wt, bt)), wo, bo)[..., 0]
        op = gain * torch.nn.functional.softplus(raw)
        best = op if best is None else torch.maximum(best, op)
    return best.reshape(B, D, H, W)


def case(name):
    if name not in _CACHE:
        kw, (n_t, n_o, hidden), size, times, r = CASES[name]
        lay = lp.kplanes_layout(**kw)
        gen = torch.Generator().manual_seed(SEEDS[name])
        shape = (size[0], lay.rows, lay.channels)   # magnitudes in [0.5, 1.5], one sign per (scene, channel), as kplanes_points_cases
        planes = (0.5 + torch.rand(shape, generator=gen)) * (torch.randint(0, 2, (size[0], 1, lay.channels), generator=gen) * 2 - 1)
        dec = random_decoder(gen, n_t, n_o, 2, lay.out_channels, hidden, 3, use_separate_color_grid=(n_t == 0), std=(2.0 / hidden) ** 0.5)
        op = oracle_opacity(planes, lay, dec, size, times, GAIN)
        t, gap = unambiguous_threshold(op)
        _CACHE[name] = dict(lay=lay, planes=planes, dec=dec, size=list(size), times=None if times is None else torch.tensor(times),
                            r=r, op=op, t=t, gap=gap)
    return _CACHE[name]


def on_device(c, dev):
    """(planes, decoder, times) of a case on ``dev``"""
    dec = c["dec"]
    ddec = lp.DecoderParams(dec.mlp_params.to(dev), dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
    return c["planes"].to(dev), ddec, None if c["times"] is None else c["times"].to(dev)

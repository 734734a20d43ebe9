"""Inputs and fp64 reference of the fused plane-field decoder (tests/test_kplanes_points_host.py holds the exclusion caps without a GPU,
tests/test_gpu_kplanes_points.py holds the kernels to the reference).  Every case is built once per process and never modified.

Reference: ``tests.test_gpu_kplanes.reference`` in fp64 on the fp32 inputs, then the decoder from the oracle's own pieces under
``relu_margin_recorder``; autograd differentiates it.  Exclusions are conditions on the fp64 inputs.  Upstream gradients are ZERO
(at most 5 % of a case) where the ReLU margin is below 1e-5, a plane coordinate (time included) is within 1e-4 of an integer on any
scale, the point is within 1e-3 of the contraction's kink, or the point is left out; a point is LEFT OUT of the value comparisons (at
most 2 %) within 1e-5 of a cube face with the mask on (a scaffold masks too) or within 1e-3 of a scaffold cell boundary.  A seed that
misses a cap is changed, never the bar."""
import torch

import lightplane_amd as lp
from oracle import lightplane_oracle as O
from tests import test_gpu_kplanes as KP
from tests.points_cases import CELL_EPS, GAIN, MAX_LEFT_OUT, MAX_ZEROED, RELU_MARGIN, _near_half, _unnorm  # noqa: F401
from tests.synth import random_decoder

DYN = KP.DYN   # n = (5, 9), m = (4, 4), C = 8
#   name: layout, (trunk, opacity, colour layers, hidden), (R, N), batch, how the points are drawn, mask, contract, scaffold shape,
#   times per point
CASES = {
    "dynamic_222x32": (DYN, (2, 2, 2, 32), (7, 37), 2, 1.2, False, False, None, False),
    "static_112x32": (dict(DYN, time_resolution=None), (1, 1, 2, 32), (7, 37), 2, 1.2, False, False, None, False),
    "c4_112x32": (dict(DYN, channels=4), (1, 1, 2, 32), (7, 37), 2, 1.2, False, False, None, False),
    "c64_112x64": (dict(DYN, time_resolution=4, channels=64), (1, 1, 2, 64), (7, 37), 2, 1.2, False, False, None, False),
    "notrunk_022x32": (dict(resolutions=(4, 8, 16, 32), time_resolution=6, channels=8), (0, 2, 2, 32), (7, 37), 2, 1.2, False, False, None,
                       False),
    "point_times": (DYN, (1, 1, 2, 32), (7, 37), 2, 1.2, False, False, None, True),
    "zeros": (DYN, (1, 1, 2, 32), (7, 37), 2, 1.2, False, False, None, False),
    # (the contraction leaves no point outside the cube: the mask at work, points outside [-1, 1]^3 that add exactly nothing)
    "masked_112x32": (DYN, (1, 1, 2, 32), (7, 37), 2, 1.2, True, False, None, False),
    "contract_mask_scaffold": (DYN, (2, 2, 2, 32), (7, 37), 1, 3.0, True, True, (1, 5, 4, 6), False),
    "one_cell": (DYN, (1, 1, 2, 32), (1, 64), 2, "cell", False, False, None, False),
    "along_ray": (DYN, (1, 1, 2, 32), (1, 200), 2, "ray", False, False, None, False),
    "one_point": (DYN, (2, 2, 2, 32), (1, 1), 2, 1.2, False, False, None, False),
    # 131 109 points = 2 049 tiles: two tiles per workgroup and a part-filled last one; the narrow decoder keeps the fp64 reference quick
    "many_tiles": (dict(resolutions=(8,), time_resolution=None, channels=4), (1, 1, 1, 8), (33, 3973), 2, 1.2, False, False, None, False),
}
SEEDS = {name: 1400 + i for i, name in enumerate(CASES)}
ALL = list(CASES)
_CACHE = {}


def case(name):
    if name in _CACHE:
        return _CACHE[name]
    kw, (n_t, n_o, n_c, hidden), (R, N), B, draw, mask, contract, sc_shape, per_point = CASES[name]
    lay = lp.kplanes_layout(**kw)
    gen = torch.Generator().manual_seed(SEEDS[name])
    # (the drawing conventions of tests/test_gpu_kplanes.py)
    if draw == "cell":    # inside cell (3, 6, 1) of the finest scale, at 0.1 .. 0.9 of the cell
        pts = 2 * (torch.tensor([3.0, 6.0, 1.0]) + 0.1 + 0.8 * torch.rand(R, N, 3, generator=gen)) / (lay.spatial[-1] - 1) - 1
    elif draw == "ray":   # sorted depths along one ray through the box
        t = torch.rand(R, N, generator=gen).sort(dim=1).values
        pts = torch.tensor([-0.9, -0.7, -0.8]) + t[..., None] * torch.tensor([1.7, 1.5, 1.2])
    else:
        pts = (torch.rand(R, N, 3, generator=gen) * 2 - 1) * draw
    times = None
    if lay.n_planes == 6:
        times = (torch.rand((R, N) if per_point else (R,), generator=gen) * 2 - 1) * 1.2
    gidx = torch.tensor([0, 1, 1, 0, 5, -2, 1])[torch.arange(R) % 7] if B > 1 else torch.zeros(R, dtype=torch.int64)
    shape = (B, lay.rows, lay.channels)   # magnitudes in [0.5, 1.5], one sign per (scene, channel): a product of six stays in range
    planes = (0.5 + torch.rand(shape, generator=gen)) * (torch.randint(0, 2, (B, 1, lay.channels), generator=gen) * 2 - 1)
    if name == "zeros":   # a third of the entries exactly 0, and every row of the xy plane of scale 0
        planes[torch.rand(shape, generator=gen) < 1 / 3] = 0.0
        planes[:, lay.offsets[0][0]:lay.offsets[0][1]] = 0.0
    dec = random_decoder(gen, n_t, n_o, n_c, lay.out_channels, hidden, 3, std=(2.0 / hidden) ** 0.5)
    enc = torch.randn(R, int(dec.n_hidden_color[0]), generator=gen)
    scaffold = None if sc_shape is None else (torch.rand(sc_shape, generator=gen) < 0.6).float()
    g_op, g_col = torch.randn(R, N, generator=gen), torch.randn(R, N, 3, generator=gen)

    # ---- where fp32 geometry may take another branch (fp64 coordinates of the fp32 points) ----
    p64, t64 = pts.double(), None if times is None else times.double()
    q64 = KP._contract(p64) if contract else p64
    left_out = torch.zeros(R, N, dtype=torch.bool)
    if scaffold is not None:
        for ax, size in ((0, sc_shape[3]), (1, sc_shape[2]), (2, sc_shape[1])):
            left_out |= _near_half(_unnorm(q64[..., ax], size), CELL_EPS)
    if mask or scaffold is not None:
        left_out |= ((q64.abs() - 1.0).abs() < KP.FACE_EPS).any(-1)
    zeroed = left_out.clone()
    if contract:
        a = p64.abs().sort(dim=-1, descending=True).values
        zeroed |= ((a[..., 0] - 1.0).abs() < KP.KINK_EPS) | ((a[..., 0] > 1.0) & ((a[..., 0] - a[..., 1]) < KP.KINK_EPS))
    for s in range(lay.n_scales):
        for c, n in zip(KP._coords(q64, t64), [lay.spatial[s]] * 3 + ([lay.temporal[s]] if lay.temporal else [])):
            x = ((c + 1) / 2 * (n - 1)).clamp(-0.5, n - 0.5)   # (a coordinate clamped away has no kink)
            zeroed |= (x - x.round()).abs() < KP.INT_EPS

    # ---- fp64 reference ----
    leaves = dict(points=p64.clone().requires_grad_(True), planes=planes.double().requires_grad_(True),
                  params=dec.mlp_params.double().requires_grad_(True), enc=enc.double().requires_grad_(True))
    (wt, bt), (wo, bo), (wc, bc) = O.split_decoder(leaves["params"], dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color)
    touched = torch.zeros(B, lay.rows, dtype=torch.bool)
    with O.relu_margin_recorder() as rec:
        feat = KP.reference(leaves["points"], t64, leaves["planes"], gidx, lay, mask, contract, touched)
        trunk = O._relu(O.mlp_forward(feat, wt, bt))
        raw = O.mlp_forward(trunk, wo, bo)[..., 0]
        craw = O.mlp_forward(trunk + leaves["enc"][:, None], wc, bc)[..., :3]
    occ = torch.ones(R, N, dtype=torch.float64)
    if scaffold is not None:
        occ = O.sample_scaffold_nearest(scaffold.double(), q64, gidx.clamp(0, B - 1))
    op, col = GAIN * torch.nn.functional.softplus(raw) * occ, torch.sigmoid(craw) * occ[..., None]
    zeroed |= rec.margin < RELU_MARGIN
    live = (~zeroed).float()
    u_op, u_col = g_op * live, g_col * live[..., None]
    (op * u_op.double()).sum().add((col * u_col.double()).sum()).backward()
    inside = (q64.abs() <= 1.0).all(-1) | (not mask)
    _CACHE[name] = dict(lay=lay, dec=dec, pts=pts, times=times, gidx=gidx, planes=planes, enc=enc, scaffold=scaffold, mask=mask,
                        contract=contract, op=op.detach(), col=col.detach(), occ=occ, left_out=left_out, zeroed=zeroed, inside=inside,
                        u_op=u_op, u_col=u_col, grads={k: v.grad for k, v in leaves.items()}, untouched=~touched)
    return _CACHE[name]


def on_device(c, dev, requires_grad=()):
    """the case's leaves on ``dev`` (those named in ``requires_grad`` ask for a gradient) and its decoder around ``params``"""
    d = {k: c[k].to(dev).requires_grad_(k in requires_grad) for k in ("planes", "enc")}
    d["points"] = c["pts"].to(dev).requires_grad_("points" in requires_grad)
    d["params"] = c["dec"].mlp_params.to(dev).requires_grad_("params" in requires_grad)
    d["times"] = None if c["times"] is None else c["times"].to(dev)
    dec = c["dec"]
    d["dec"] = lp.DecoderParams(d["params"], dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
    return d


def evaluate(c, d, opacity_only=False, **over):
    """the fused op on the tensors ``d`` of ``on_device`` (``over``: other points / times / gidx / enc)"""
    dev = d["points"].device
    pts, times, gidx = over.get("points", d["points"]), over.get("times", d["times"]), over.get("gidx", c["gidx"].to(dev))
    kw = dict(mask_out_of_bounds_samples=c["mask"], contract_coords=c["contract"],
              scaffold=None if c["scaffold"] is None else c["scaffold"].to(dev))
    if opacity_only:
        return lp.kplanes_eval_mlp_opacity_only(pts, times, d["planes"], gidx, c["lay"], d["dec"], GAIN, **kw)
    return lp.kplanes_eval_mlp(pts, times, d["planes"], gidx, c["lay"], d["dec"], over.get("enc", d["enc"]), GAIN, **kw)

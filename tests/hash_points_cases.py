"""Inputs and fp64 reference of the fused hash-grid decoder (tests/test_hash_points_host.py holds the exclusion caps without a GPU,
tests/test_gpu_hash_points.py holds the kernels to the reference).  Every case is built once per process and never modified.

Reference: ``tests.test_gpu_hash_grid.reference`` in fp64 on the fp32 inputs, then the decoder from the oracle's own pieces under
``relu_margin_recorder``; autograd differentiates it.  Exclusions are conditions on the fp64 inputs.  Upstream gradients are ZERO
(at most 5 % of a case) where the ReLU margin is below 1e-5, x = (q + 1) / 2 N_l is within 1e-4 of an integer on any level and
axis, the point is within 1e-3 of the contraction's kink, or the point is left out; a point is LEFT OUT of the value comparisons (at
most 2 %) within 1e-5 of a cube face with the mask on (a scaffold masks too) or within 1e-3 of a scaffold cell boundary.  A seed that
misses a cap is changed, never the bar."""
import torch

import lightplane_amd as lp
from oracle import lightplane_oracle as O
from tests import test_gpu_hash_grid as HG
from tests.points_cases import CELL_EPS, GAIN, MAX_LEFT_OUT, MAX_ZEROED, RELU_MARGIN, _near_half, _unnorm  # noqa: F401
from tests.synth import random_decoder

MIXED = HG.MIXED   # L = 4, F = 2, T = 2^8, 4 -> 32: one dense level, three hashed ones
#   name: layout, (trunk, opacity, colour layers, hidden), (R, N), batch, how the points are drawn, mask, contract, scaffold shape
CASES = {
    "mixed_222x32": (MIXED, (2, 2, 2, 32), (7, 37), 2, 1.2, False, False, None),
    "f1_112x32": (dict(MIXED, features_per_level=1), (1, 1, 2, 32), (7, 37), 2, 1.2, False, False, None),
    "f8_112x64": (dict(MIXED, features_per_level=8), (1, 1, 2, 64), (7, 37), 2, 1.2, False, False, None),
    "ngp_022x32": (dict(n_levels=16, features_per_level=2, log2_table_size=10, base_resolution=16, finest_resolution=256), (0, 2, 2, 32),
                   (7, 37), 2, 1.2, False, False, None),
    "contract_mask_scaffold": (MIXED, (2, 2, 2, 32), (7, 37), 1, 3.0, True, True, (1, 5, 4, 6)),
    "one_cell": (MIXED, (1, 1, 2, 32), (1, 64), 1, "cell", False, False, None),
    "along_ray": (dict(MIXED, n_levels=3, base_resolution=2, finest_resolution=8), (1, 1, 2, 32), (1, 200), 1, "ray", False, False, None),
    "many_tiles": (dict(MIXED, n_levels=2, base_resolution=8, finest_resolution=32), (1, 1, 2, 32), (33, 3973), 2, 1.2, False, False, None),
    "one_point": (MIXED, (2, 2, 2, 32), (1, 1), 2, 1.2, False, False, None),
    # (the contraction leaves no point outside the cube: the mask at work, points outside [-1, 1]^3 that add exactly nothing)
    "masked_112x32": (MIXED, (1, 1, 2, 32), (7, 37), 2, 1.2, True, False, None),
    # 918 017 points = 14 345 tiles: 8 tiles per workgroup, the most a test reaches, and a part-filled last one; the narrowest decoder
    # keeps the fp64 reference quick
    "eight_tiles": (dict(MIXED, n_levels=2, features_per_level=1, base_resolution=8, finest_resolution=32), (1, 1, 1, 8), (17, 54001), 2,
                    1.2, False, False, None),
}
SEEDS = {name: 1200 + i for i, name in enumerate(CASES)}
ALL = list(CASES)
_CACHE = {}


def case(name):
    if name in _CACHE:
        return _CACHE[name]
    kw, (n_t, n_o, n_c, hidden), (R, N), B, draw, mask, contract, sc_shape = CASES[name]
    lay = lp.hash_grid_layout(**kw)
    gen = torch.Generator().manual_seed(SEEDS[name])
    if draw == "cell":    # inside cell (10, 20, 5) of the finest level, away from its faces
        pts = 2 * (torch.tensor([10.0, 20.0, 5.0]) + 0.1 + 0.8 * torch.rand(R, N, 3, generator=gen)) / lay.resolutions[-1] - 1
    elif draw == "ray":   # sorted depths along one ray through the box
        t = torch.rand(R, N, generator=gen).sort(dim=1).values
        pts = torch.tensor([-0.9, -0.7, -0.8]) + t[..., None] * torch.tensor([1.7, 1.5, 1.2])
    else:
        pts = (torch.rand(R, N, 3, generator=gen) * 2 - 1) * draw
    gidx = torch.tensor([0, 1, 1, 0, 5, -2, 1])[torch.arange(R) % 7] if B > 1 else torch.zeros(R, dtype=torch.int64)
    table = torch.randn(B, lay.entries, lay.features_per_level, generator=gen)
    dec = random_decoder(gen, n_t, n_o, n_c, lay.channels, hidden, 3, std=(2.0 / hidden) ** 0.5)
    enc = torch.randn(R, int(dec.n_hidden_color[0]), generator=gen)
    scaffold = None if sc_shape is None else (torch.rand(sc_shape, generator=gen) < 0.6).float()
    g_op, g_col = torch.randn(R, N, generator=gen), torch.randn(R, N, 3, generator=gen)

    # ---- where fp32 geometry may take another branch (fp64 coordinates of the fp32 points) ----
    p64 = pts.double()
    q64 = HG._contract(p64) if contract else p64
    left_out = torch.zeros(R, N, dtype=torch.bool)
    if scaffold is not None:
        for ax, size in ((0, sc_shape[3]), (1, sc_shape[2]), (2, sc_shape[1])):
            left_out |= _near_half(_unnorm(q64[..., ax], size), CELL_EPS)
    if mask or scaffold is not None:
        left_out |= ((q64.abs() - 1.0).abs() < HG.FACE_EPS).any(-1)
    zeroed = left_out.clone()
    if contract:
        a = p64.abs().sort(dim=-1, descending=True).values
        zeroed |= ((a[..., 0] - 1.0).abs() < HG.KINK_EPS) | ((a[..., 0] > 1.0) & ((a[..., 0] - a[..., 1]) < HG.KINK_EPS))
    for n_l in lay.resolutions:
        x = ((q64 + 1) / 2 * n_l).clamp(-0.5, n_l + 0.5)   # (a coordinate clamped away has no kink)
        zeroed |= ((x - x.round()).abs() < HG.INT_EPS).any(-1)

    # ---- fp64 reference ----
    leaves = dict(points=p64.clone().requires_grad_(True), table=table.double().requires_grad_(True),
                  params=dec.mlp_params.double().requires_grad_(True), enc=enc.double().requires_grad_(True))
    (wt, bt), (wo, bo), (wc, bc) = O.split_decoder(leaves["params"], dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color)
    with O.relu_margin_recorder() as rec:
        feat = HG.reference(leaves["points"], leaves["table"], gidx, lay, mask, contract)
        trunk = O._relu(O.mlp_forward(feat, wt, bt))
        raw = O.mlp_forward(trunk, wo, bo)[..., 0]
        craw = O.mlp_forward(trunk + leaves["enc"][:, None], wc, bc)[..., :3]
    occ = torch.ones(R, N, dtype=torch.float64)
    if scaffold is not None:
        occ = O.sample_scaffold_nearest(scaffold.double(), q64, gidx.clamp(0, B - 1))
    op, col = GAIN * torch.nn.functional.softplus(raw) * occ, torch.sigmoid(craw) * occ[..., None]
    (touched,) = torch.autograd.grad(feat, leaves["table"], torch.ones_like(feat), retain_graph=True)   # (the weights are >= 0)
    zeroed |= rec.margin < RELU_MARGIN
    live = (~zeroed).float()
    u_op, u_col = g_op * live, g_col * live[..., None]
    (op * u_op.double()).sum().add((col * u_col.double()).sum()).backward()
    inside = (q64.abs() <= 1.0).all(-1) | (not mask)
    _CACHE[name] = dict(lay=lay, dec=dec, pts=pts, gidx=gidx, table=table, enc=enc, scaffold=scaffold, mask=mask, contract=contract,
                        op=op.detach(), col=col.detach(), occ=occ, left_out=left_out, zeroed=zeroed, inside=inside, u_op=u_op, u_col=u_col,
                        grads={k: v.grad for k, v in leaves.items()}, untouched=touched == 0)
    return _CACHE[name]


def on_device(c, dev, requires_grad=()):
    """the case's leaves on ``dev`` (those named in ``requires_grad`` ask for a gradient) and its decoder around ``params``"""
    d = {k: c[k].to(dev).requires_grad_(k in requires_grad) for k in ("table", "enc")}
    d["points"] = c["pts"].to(dev).requires_grad_("points" in requires_grad)
    d["params"] = c["dec"].mlp_params.to(dev).requires_grad_("params" in requires_grad)
    dec = c["dec"]
    d["dec"] = lp.DecoderParams(d["params"], dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
    return d


def evaluate(c, d, opacity_only=False, **over):
    """the fused op on the tensors ``d`` of ``on_device`` (``over``: other points / table / gidx)"""
    dev = d["points"].device
    pts, table, gidx = over.get("points", d["points"]), over.get("table", d["table"]), over.get("gidx", c["gidx"].to(dev))
    kw = dict(mask_out_of_bounds_samples=c["mask"], contract_coords=c["contract"],
              scaffold=None if c["scaffold"] is None else c["scaffold"].to(dev))
    if opacity_only:
        return lp.hash_grid_eval_mlp_opacity_only(pts, table, gidx, c["lay"], d["dec"], GAIN, **kw)
    return lp.hash_grid_eval_mlp(pts, table, gidx, c["lay"], d["dec"], over.get("enc", d["enc"]), GAIN, **kw)

"""Inputs and fp64 oracle of the point-evaluation tests (tests/test_points_host.py checks the inputs without a GPU,
tests/test_gpu_points.py holds the kernels to the oracle).  Every case is built once per process and never modified.

Oracle: ``oracle.lightplane_oracle.eval_decoder`` in fp64 on the fp32 inputs, differentiated with autograd.

Points left out of the VALUE comparison (fp32 geometry may legitimately pick the other side of a jump there; at most 2 % of a case):
* within 1e-3 of a cell of a scaffold cell boundary (the nearest-neighbour lookup rounds the un-normalised coordinate);
* within 1e-5 of a face of [-1, 1]^3 when the out-of-bounds mask is on (a scaffold masks out-of-bounds points too).

Points whose upstream gradient is set to ZERO (the derivative is not defined to fp32 accuracy there; everything is linear in the
upstream gradient per point, so such a point contributes to no gradient, in the kernel and in the oracle alike; at most 5 % of a case):
* ``relu_margin_recorder`` margin < 1e-5 (ten times the kernels' pre-activation round-off; the suite's TIE_EPS is 1e-6);
* within 1e-3 of a cell of a cell face of any grid of either grid-list (the interpolation weights have a kink there);
* within 1e-3 of the kink of ``contract_pi``: max |p_j| = 1, or two coordinates sharing the maximum beyond it;
* the points left out of the value comparison (the other side of a jump is another branch: another gradient).
A seed that misses a cap is changed, never the bar.
"""
import torch

import lightplane_amd as lp
from oracle import lightplane_oracle as O
from tests.synth import grid_sizes_for, random_decoder

GAIN = 1.7
TOL = 1e-4          # the project's bar: max |err| / max |ref|
RELU_MARGIN = 1e-5
CELL_EPS = 1e-3     # of a cell
FACE_EPS = 1e-5
MAX_LEFT_OUT = 0.02
MAX_ZEROED = 0.05

#   name: grid kind, base [B, D, H, W, C], (trunk, opacity, colour layers, hidden), (R, N), grid form, contract, mask, scaffold shape
CASES = {
    "triplane_c16_222x32": ("triplane", (2, 6, 5, 7, 16), (2, 2, 2, 32), (7, 37), "list", False, False, None),
    "voxel_c32_112x64_flat": ("voxel", (2, 4, 3, 5, 32), (1, 1, 2, 64), (7, 37), "flat", False, False, None),
    "voxel_c32_twogrid_022x32": ("voxel", (2, 5, 4, 6, 32), (0, 2, 2, 32), (7, 37), "list", False, False, None),
    "triplane_c16_322x64_contract_mask_scaffold": ("triplane", (1, 8, 7, 9, 16), (3, 2, 2, 64), (7, 37), "list", True, True, (1, 5, 4, 6)),
    "triplane_c16_222x128": ("triplane", (2, 6, 5, 7, 16), (2, 2, 2, 128), (3, 70), "list", False, False, None),
    "triplane_c16_222x32_one_point": ("triplane", (2, 6, 5, 7, 16), (2, 2, 2, 32), (1, 1), "list", False, False, None),
    "voxel_c16_112x32_one_wave": ("voxel", (1, 4, 3, 5, 16), (1, 1, 2, 32), (1, 64), "list", False, False, None),
    # ragged widths (tests/ragged_cases.py): scalar grid rows and layers narrower than a block of eight; full blocks and one output
    "voxel_c5_222x7_mask": ("voxel", (2, 4, 3, 5, 5), (2, 2, 2, 7), (7, 37), "list", False, True, None),
    "triplane_c20_222x33_scaffold": ("triplane", (1, 6, 5, 7, 20), (2, 2, 2, 33), (7, 37), "flat", False, False, (1, 5, 4, 6)),
}
SEEDS = {name: 300 + i for i, name in enumerate(CASES)}
_CACHE = {}


def _unnorm(c, size):
    return ((c + 1) * size - 1) / 2


def _near_half(t, eps):
    """|t - (k + 0.5)| < eps for some integer k: a rounding boundary of the nearest-neighbour lookup"""
    return ((t - torch.floor(t)) - 0.5).abs() < eps


def _near_int(t, eps):
    return (t - torch.round(t)).abs() < eps


def _double_decoder(dec, params):
    return lp.DecoderParams(params, dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)


def case(name, decoder_transform=None, key=None):
    """``decoder_transform`` (tests/value_regime_cases.py): the case with ``decoder_transform(decoder)`` in place of its decoder, cached
    under ``key``; everything else -- grids, points, encoding, upstream gradients -- is the case's own."""
    assert (decoder_transform is None) == (key is None)
    key = name if key is None else key
    if key in _CACHE:
        return _CACHE[key]
    kind, base, (n_t, n_o, n_c, hidden), (R, N), form, contract, mask, sc_shape = CASES[name]
    gen = torch.Generator().manual_seed(SEEDS[name])
    B, C = base[0], base[4]
    sizes = grid_sizes_for(base, kind == "triplane")
    two = n_t == 0
    grids = [0.5 * torch.randn(s, generator=gen) for s in sizes]
    cgrids = [0.5 * torch.randn(s, generator=gen) for s in sizes] if two else None
    dec = random_decoder(gen, n_t, n_o, n_c, C, hidden, 3, use_separate_color_grid=two, std=(2.0 / hidden) ** 0.5)
    if decoder_transform is not None:
        dec = decoder_transform(dec)
    half = 3.0 if contract else 1.2
    pts = (torch.rand(R, N, 3, generator=gen) * 2 - 1) * half
    gidx = torch.randint(0, B, (R,), generator=gen)
    enc = torch.randn(R, int(dec.n_hidden_color[0]), generator=gen)
    scaffold = None if sc_shape is None else (torch.rand(sc_shape, generator=gen) < 0.6).float()
    g_op = torch.randn(R, N, generator=gen)
    g_col = torch.randn(R, N, 3, generator=gen)

    # ---- where fp32 geometry may take another branch (fp64 coordinates of the fp32 points) ----
    p64 = pts.double()
    q64 = O.contract_pi(p64) if contract else p64
    left_out = torch.zeros(R, N, dtype=torch.bool)
    if scaffold is not None:
        for ax, size in ((0, sc_shape[3]), (1, sc_shape[2]), (2, sc_shape[1])):
            left_out |= _near_half(_unnorm(q64[..., ax], size), CELL_EPS)
    if mask or scaffold is not None:
        left_out |= ((q64.abs() - 1.0).abs() < FACE_EPS).any(-1)
    on_face = torch.zeros(R, N, dtype=torch.bool)
    for s in sizes:
        for ax, size in ((0, s[3]), (1, s[2]), (2, s[1])):
            if size > 1:
                on_face |= _near_int(_unnorm(q64[..., ax], size), CELL_EPS)
    on_kink = torch.zeros(R, N, dtype=torch.bool)
    if contract:
        a = p64.abs().sort(dim=-1, descending=True).values
        on_kink = ((a[..., 0] - 1.0).abs() < CELL_EPS) | ((a[..., 0] > 1.0) & ((a[..., 0] - a[..., 1]) < CELL_EPS))

    # ---- fp64 oracle, values ----
    leaves = dict(points=p64.clone().requires_grad_(True), params=dec.mlp_params.double().requires_grad_(True),
                  enc=enc.double().requires_grad_(True), grids=[g.double().requires_grad_(True) for g in grids],
                  cgrids=None if cgrids is None else [g.double().requires_grad_(True) for g in cgrids])
    with O.relu_margin_recorder() as rec, O.value_recorder() as seen:
        op, col = O.eval_decoder(leaves["points"], leaves["grids"], gidx, _double_decoder(dec, leaves["params"]), leaves["enc"], GAIN,
                                 mask_out_of_bounds_samples=mask, scaffold=None if scaffold is None else scaffold.double(),
                                 color_grids=leaves["cgrids"], contract_coords=contract)
    col = col[..., :3]
    near_tie = rec.margin < RELU_MARGIN
    zeroed = near_tie | on_face | on_kink | left_out
    live = (~zeroed).double()
    u_op, u_col = g_op * live.float(), g_col * live.float()[..., None]

    # ---- fp64 oracle, gradients ----
    (op * u_op.double()).sum().add((col * u_col.double()).sum()).backward()
    grads = dict(points=leaves["points"].grad, params=leaves["params"].grad, enc=leaves["enc"].grad,
                 grids=[g.grad for g in leaves["grids"]], cgrids=None if cgrids is None else [g.grad for g in leaves["cgrids"]])
    _CACHE[key] = dict(name=name, grids=grids, cgrids=cgrids, dec=dec, pts=pts, gidx=gidx, enc=enc, scaffold=scaffold, form=form,
                       contract=contract, mask=mask, op=op.detach(), col=col.detach(), left_out=left_out, zeroed=zeroed,
                       counts=dict(near_tie=int(near_tie.sum()), on_face=int(on_face.sum()), on_kink=int(on_kink.sum()),
                                   left_out=int(left_out.sum())),
                       u_op=u_op, u_col=u_col, grads=grads, raw_o=seen.raw_o, raw_c=seen.raw_c[..., :3])
    return _CACHE[key]


def on_device(c, dev, requires_grad=()):
    """The case's tensors on ``dev`` in the case's grid form: dict with ``grid`` / ``color_grid`` (list or flat), their sizes, the
    decoder and the leaves named in ``requires_grad`` ("points", "params", "enc", "grids", "cgrids") made to require a gradient."""
    def leaf(t, name):
        t = t.to(dev)
        return t.requires_grad_(True) if name in requires_grad else t

    def grid_arg(gs, name):
        if gs is None:
            return None, None
        if c["form"] == "flat":
            C = gs[0].shape[-1]
            return leaf(torch.cat([g.reshape(-1, C) for g in gs]), name), [list(g.shape) for g in gs]
        return [leaf(g, name) for g in gs], None

    grid, sizes = grid_arg(c["grids"], "grids")
    cgrid, csizes = grid_arg(c["cgrids"], "cgrids")
    dec = c["dec"]
    params = leaf(dec.mlp_params, "params")
    return dict(grid=grid, sizes=sizes, color_grid=cgrid, color_sizes=csizes, params=params,
                dec=lp.DecoderParams(params, dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn),
                pts=leaf(c["pts"], "points"), gidx=c["gidx"].to(dev), enc=leaf(c["enc"], "enc"),
                scaffold=None if c["scaffold"] is None else c["scaffold"].to(dev))


def flat_grad(c, grads):
    """oracle grid gradients in the case's grid form (a list of tensors, or the flat tensor's twin as a one-entry list)"""
    if grads is None:
        return None
    if c["form"] == "flat":
        C = grads[0].shape[-1]
        return [torch.cat([g.reshape(-1, C) for g in grads])]
    return list(grads)

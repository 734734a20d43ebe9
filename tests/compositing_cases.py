"""fp64 definitions and case table of the modular march (``lightplane_amd.ray_samples`` / ``composite_samples``):
tests/test_compositing_host.py checks the definitions without a GPU, tests/test_gpu_compositing.py holds the kernels to them.

Compositing is lines 569-581 of oracle/lightplane_oracle.py (``lightplane_renderer_naive`` behind the decoder) restated on explicit
per-sample tensors, in the dtype of its inputs; gradients by autograd.  ``closed_form_gradients`` is the formula the backward kernel
implements; the host test holds it to autograd in fp64.  Sample placement is the oracle's own ``ray_depths`` / ``ray_deltas``.

The bar is the project's: max |err| / max |ref| <= ``points_cases.TOL`` per tensor, no entry left out (compositing has no ReLU and no
cell boundary).  Inputs are built once per process and never modified.
"""
import torch

from oracle import lightplane_oracle as O
from tests.points_cases import TOL  # noqa: F401  (the bar, re-exported)

RS = (1, 63, 130)
SS = (1, 2, 63, 64, 65, 131, 200)
CS = (0, 1, 3, 4, 5, 32, 64, 67, 128)
REGIMES = ("transparent", "opaque", "mixed")


def _table():
    """a covering subset of RS x SS x CS: every S with four or five channel counts (every C four times at least), every R with every
    S, both corners"""
    cases = []
    for i, S in enumerate(SS):
        for j in range(4):
            C = CS[(4 * i + j) % len(CS)]
            cases.append((RS[(i + j) % len(RS)], S, C))
    for extra in ((130, 200, 128), (1, 1, 0), (130, 1, 67), (63, 65, 128), (1, 200, 3)):
        if extra not in cases:
            cases.append(extra)
    return cases


CASES = _table()
_CACHE = {}


def composite(opacity, features, depths, deltas):
    """(ray_length, -log T, feature or None, weights) in the dtype of the inputs"""
    od = opacity * deltas
    nlt = torch.cumsum(torch.nn.functional.pad(od, (1, 0)), dim=-1)
    transmittance = torch.exp(-nlt)
    w = transmittance[:, :-1] - transmittance[:, 1:]
    ray_length = (depths * w).sum(dim=-1)
    feature = None if features is None else (features * w[..., None]).sum(dim=-2)
    return ray_length, nlt[:, -1], feature, w


def closed_form_gradients(opacity, features, depths, deltas, g_len, g_nlt, g_feat, g_w):
    """(d opacity, d features or None, d depths, d deltas): the backward kernel's formula, in the dtype of the inputs"""
    od = opacity * deltas
    nlt = torch.cumsum(torch.nn.functional.pad(od, (1, 0)), dim=-1)
    T = torch.exp(-nlt)
    w = T[:, :-1] * (-torch.expm1(-od))
    v = g_len[:, None] * depths + g_w
    if features is not None:
        v = v + (features * g_feat[:, None, :]).sum(-1)
    wv = w * v
    behind = wv.flip(-1).cumsum(-1).flip(-1) - wv  # sum over s > j
    d_od = T[:, 1:] * v - behind + g_nlt[:, None]
    d_feat = None if features is None else w[..., None] * g_feat[:, None, :]
    return d_od * deltas, d_feat, g_len[:, None] * w, d_od * opacity


def inputs(R, S, C, regime, seed=None):
    """fp32 inputs and upstream gradients of one case.  deltas in [0.01, 0.06], depths their running sum from 0.5.
    transparent: -log T of the whole ray about 0.05; opaque: about 50, reached within three samples; mixed: moderate opacities, every
    third row all zero and row 0 with opacity 1e6 from its middle sample on (T underflows to 0 there)."""
    gen = torch.Generator().manual_seed(1000 * R + 10 * S + C + 7 * REGIMES.index(regime) if seed is None else seed)
    deltas = torch.rand(R, S, generator=gen) * 0.05 + 0.01
    depths = 0.5 + torch.cumsum(deltas, -1)
    u = torch.rand(R, S, generator=gen)
    if regime == "transparent":
        opacity = u * (2 * 0.05 / (S * 0.035))
    elif regime == "opaque":
        opacity = u * 5.0
        k = min(S, 3)
        opacity[:, :k] = (50.0 / k) / deltas[:, :k]
    else:
        opacity = u * 2.0
        opacity[1::3] = 0.0
        opacity[0, S // 2:] = 1e6
    features = torch.randn(R, S, C, generator=gen) if C > 0 else None
    ups = dict(g_len=torch.randn(R, generator=gen), g_nlt=torch.randn(R, generator=gen),
               g_feat=torch.randn(R, C, generator=gen) if C > 0 else None, g_w=torch.randn(R, S, generator=gen))
    return dict(opacity=opacity, features=features, depths=depths, deltas=deltas, **ups)


def case(R, S, C, regime):
    """the inputs with their fp64 results and gradients, with (``grads_w``) and without (``grads``) an upstream gradient on the weights"""
    key = (R, S, C, regime)
    if key in _CACHE:
        return _CACHE[key]
    c = inputs(R, S, C, regime)
    d = {k: (None if v is None else v.double()) for k, v in c.items()}
    for with_w in (False, True):
        leaves = [d[k].clone().requires_grad_(True) if d[k] is not None else None for k in ("opacity", "features", "depths", "deltas")]
        length, nlt, feature, w = composite(*leaves)
        loss = (length * d["g_len"]).sum() + (nlt * d["g_nlt"]).sum()
        if feature is not None:
            loss = loss + (feature * d["g_feat"]).sum()
        if with_w:
            loss = loss + (w * d["g_w"]).sum()
        loss.backward()
        c["grads_w" if with_w else "grads"] = [None if t is None else t.grad for t in leaves]
    c["out"] = tuple(None if t is None else t.detach() for t in (length, nlt, feature, w))
    _CACHE[key] = c
    return c


def placement(rays, num_samples, num_samples_inf, disparity_at_inf, dtype):
    """(points, depths, deltas) of the oracle's formulas in ``dtype`` (fp32: the formulas the kernels restate operation by operation)"""
    near, far = rays.near.to(dtype), rays.far.to(dtype)
    depths = O.ray_depths(near, far, num_samples, num_samples_inf, disparity_at_inf)
    deltas = O.ray_deltas(near, far, depths, num_samples)
    points = depths[..., None] * rays.directions.to(dtype)[:, None] + rays.origins.to(dtype)[:, None]
    return points, depths, deltas


# ------------------------------------------------------------------------------------------------------------------------------
# the chain ray_samples -> lightplane_eval_mlp -> composite_samples against the Renderer's oracle
# ------------------------------------------------------------------------------------------------------------------------------
#   name: triplane?, grid base [B, D, H, W, C], contract_coords, seed (picked on the CPU: test_compositing_host.py holds it to the cap)
CHAIN_CASES = {
    "triplane": (True, (2, 8, 7, 9, 16), False, 11),
    "triplane_contract": (True, (2, 8, 7, 9, 16), True, 12),
    "voxel": (False, (2, 6, 5, 7, 16), False, 13),
    "voxel_contract": (False, (2, 6, 5, 7, 16), True, 14),
}
CHAIN_RAYS, CHAIN_S, CHAIN_S_INF, CHAIN_GAIN, CHAIN_DISPARITY = 130, 65, 3, 1.7, 1e-5


def chain_case(name):
    """Inputs, the fp64 results of ``lightplane_renderer_naive`` and the fp64 gradients of the chain with respect to origins,
    directions, near and far (and, as the decoder's own tests do, to the grids and the decoder's parameters).

    The gradients come from autograd through the oracle's own pieces -- ``ray_depths`` / ``ray_deltas``, ``eval_decoder`` and the
    compositing above, which together are ``lightplane_renderer_naive`` (asserted: the same three results to 1e-12).  Decoder kinks are
    excluded by the rules of tests/points_cases.py: at a sample (``kink``) whose ReLU margin is below ``RELU_MARGIN``, that lies within
    ``CELL_EPS`` of a cell of a cell face of a grid, or within ``CELL_EPS`` of the kink of the contraction, the decoder's derivative
    with respect to the point is not defined to fp32 accuracy, and the point is detached there -- in the oracle and, by the test, in
    the chain alike.  At most ``MAX_LEFT_OUT`` of the samples."""
    from tests import points_cases as PC
    from tests.synth import grid_sizes_for, random_decoder, random_rays
    import lightplane_amd as lp

    key = ("chain", name)
    if key in _CACHE:
        return _CACHE[key]
    triplane, base, contract, seed = CHAIN_CASES[name]
    gen = torch.Generator().manual_seed(seed)
    B, C = base[0], base[4]
    sizes = grid_sizes_for(base, triplane)
    grids = [0.5 * torch.randn(s, generator=gen) for s in sizes]
    dec = random_decoder(gen, 2, 2, 2, C, 32, 3, std=(2.0 / 32) ** 0.5)
    rays = random_rays(gen, CHAIN_RAYS, B, 32)
    ups = (torch.randn(CHAIN_RAYS, generator=gen), torch.randn(CHAIN_RAYS, generator=gen), torch.randn(CHAIN_RAYS, 3, generator=gen))

    p64 = dec.mlp_params.double().requires_grad_(True)
    dec64 = lp.DecoderParams(p64, dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
    g64 = [g.double().requires_grad_(True) for g in grids]
    leaves = {k: getattr(rays, k).double().clone().requires_grad_(True) for k in ("origins", "directions", "near", "far")}
    r64 = lp.Rays(directions=leaves["directions"], origins=leaves["origins"], grid_idx=rays.grid_idx, near=leaves["near"],
                  far=leaves["far"], encoding=rays.encoding.double())
    points, depths, deltas = placement(r64, CHAIN_S, CHAIN_S_INF, CHAIN_DISPARITY, torch.float64)

    # ---- where fp32 geometry may take another branch of the decoder ----
    with torch.no_grad():
        p = points.detach()
        q = O.contract_pi(p) if contract else p
        on_face = torch.zeros(p.shape[:2], dtype=torch.bool)
        for s in sizes:
            for ax, size in ((0, s[3]), (1, s[2]), (2, s[1])):
                if size > 1:
                    on_face |= PC._near_int(PC._unnorm(q[..., ax], size), PC.CELL_EPS)
        on_kink = torch.zeros_like(on_face)
        if contract:
            a = p.abs().sort(dim=-1, descending=True).values
            on_kink = ((a[..., 0] - 1.0).abs() < PC.CELL_EPS) | ((a[..., 0] > 1.0) & ((a[..., 0] - a[..., 1]) < PC.CELL_EPS))
        with O.relu_margin_recorder() as rec:
            O.eval_decoder(p, g64, rays.grid_idx, dec64, r64.encoding, CHAIN_GAIN, contract_coords=contract)
        kink = (rec.margin < PC.RELU_MARGIN) | on_face | on_kink

    live = torch.where(kink[..., None], points.detach(), points)
    opacity, color = O.eval_decoder(live, g64, rays.grid_idx, dec64, r64.encoding, CHAIN_GAIN, contract_coords=contract)
    length, nlt, feature, _ = composite(opacity, color[..., :3], depths, deltas)
    ((length * ups[0].double()).sum() + (nlt * ups[1].double()).sum() + (feature * ups[2].double()).sum()).backward()
    with torch.no_grad():
        want = O.lightplane_renderer_naive(r64, g64, dec64, CHAIN_S, CHAIN_GAIN, num_samples_inf=CHAIN_S_INF, contract_coords=contract,
                                           disparity_at_inf=CHAIN_DISPARITY)
    for a, b in zip((length, nlt, feature), want):
        assert float((a.detach() - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), "the pieces are not the oracle Renderer"
    _CACHE[key] = dict(name=name, grids=grids, dec=dec, rays=rays, contract=contract, ups=ups, kink=kink,
                       counts=dict(on_face=int(on_face.sum()), on_kink=int(on_kink.sum()), near_tie=int((rec.margin < PC.RELU_MARGIN).sum())),
                       out=tuple(t.detach() for t in want),
                       grads=dict({k: v.grad for k, v in leaves.items()}, grids=[g.grad for g in g64], mlp_params=p64.grad))
    return _CACHE[key]

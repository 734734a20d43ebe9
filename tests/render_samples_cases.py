"""Case table and fp64 definition of ``lightplane_amd.render_samples`` (decoder + compositing at caller-given depths):
tests/test_render_samples_host.py checks the definition without a GPU, tests/test_gpu_render_samples.py holds the kernels to it.

Definition: ``oracle.lightplane_oracle.eval_decoder`` at ``depths * direction + origin`` followed by ``compositing_cases.composite``,
in the dtype of its inputs; gradients by autograd.  At the depths of ``ray_samples`` it is ``lightplane_renderer_naive`` (held to 1e-12
by the host test).

Shapes are those of tests/points_cases.py (its table's grids, decoders, grid forms, flags and scaffolds, built with its generators);
the ragged one runs without its out-of-bounds mask so that it takes part in the comparison with fp64.  Sizes: a covering subset of
``RS x SS`` in the manner of ``compositing_cases._table``.

Depth regimes (the GPU test takes the depths from the library's own sample ops, so that the chain it compares with reads the points
those ops wrote):
  uniform     ``ray_samples(rays, S)``
  beyond_far  ``ray_samples(rays, S - k, k)``, k = min(3, S - 1) samples beyond ``far``, rendered with ``contract_coords``: the deltas grow
              by orders of magnitude
  resampled   ``importance_samples`` of ``S - S // 3`` new samples on ``S // 3`` coarse ones (S >= 9) from a weight row with one peak whose
              bin has zero width (``peaked_depths``): runs of equal depths and zero deltas
  zero        the uniform depths with every delta 0
Opacity regimes, set through ``gain`` from the fp64 opacities at gain 1 (the opacity is linear in it): ``transparent`` -- the median
``-log T`` of the batch is 0.05; ``mixed`` -- gain 1.7; ``opaque`` -- the median ``-log T`` is 800, so that T underflows (``-log T`` > 104
in fp32) in the first quarter of a typical ray.  Where every ``-log T`` is 0 (the ``zero`` regime) the gain is 1.7.
"""
import torch

import lightplane_amd as lp
from oracle import lightplane_oracle as O
from tests import compositing_cases as CC
from tests import points_cases as PC
from tests.synth import grid_sizes_for, random_decoder, random_rays

TOL = PC.TOL
RS = (1, 9, 130)
SS = (1, 2, 63, 64, 65, 130, 200)
DEPTHS = ("uniform", "beyond_far", "resampled", "zero")
OPACITIES = ("transparent", "mixed", "opaque")
DISPARITY = 1e-5

#   name: the row of points_cases.CASES whose grid, decoder, form and flags it takes, mask override (None = the row's)
SHAPES = {
    "triplane_c16_222x32": ("triplane_c16_222x32", None),
    "voxel_c32_112x64_flat": ("voxel_c32_112x64_flat", None),
    "voxel_c32_twogrid_022x32": ("voxel_c32_twogrid_022x32", None),
    "triplane_c16_322x64_contract_mask_scaffold": ("triplane_c16_322x64_contract_mask_scaffold", None),
    "triplane_c16_222x128": ("triplane_c16_222x128", None),
    "voxel_c5_222x7": ("voxel_c5_222x7_mask", False),
}
_SCENES, _RAYS = {}, {}


def scene(name):
    """grids, colour grids, decoder, scaffold, grid form and flags of a shape; built once, never modified (the dictionary has the
    keys ``points_cases.on_device`` reads)"""
    if name in _SCENES:
        return _SCENES[name]
    row, mask_override = SHAPES[name]
    kind, base, (n_t, n_o, n_c, hidden), _, form, contract, mask, sc_shape = PC.CASES[row]
    gen = torch.Generator().manual_seed(700 + list(SHAPES).index(name))
    C = base[4]
    sizes = grid_sizes_for(base, kind == "triplane")
    two = n_t == 0
    grids = [0.5 * torch.randn(s, generator=gen) for s in sizes]
    cgrids = [0.5 * torch.randn(s, generator=gen) for s in sizes] if two else None
    dec = random_decoder(gen, n_t, n_o, n_c, C, hidden, 3, use_separate_color_grid=two, std=(2.0 / hidden) ** 0.5)
    scaffold = None if sc_shape is None else (torch.rand(sc_shape, generator=gen) < 0.6).float()
    _SCENES[name] = dict(name=name, B=base[0], grids=grids, cgrids=cgrids, dec=dec, scaffold=scaffold, form=form, contract=contract,
                         mask=mask if mask_override is None else mask_override, enc_dim=int(dec.n_hidden_color[0]),
                         jumps=(mask if mask_override is None else mask_override) or scaffold is not None)
    return _SCENES[name]


def rays_for(name, R):
    """the ``R`` rays of a shape (origins inside the scene, directions through it, near about 0.1, far about 3), with an encoding"""
    key = (name, R)
    if key not in _RAYS:
        sc = scene(name)
        _RAYS[key] = random_rays(torch.Generator().manual_seed(900 + 7 * R + list(SHAPES).index(name)), R, sc["B"], sc["enc_dim"])
    return _RAYS[key]


def _table():
    """every S with three shapes (every shape three times at least), every R with every S, every depth regime with every opacity
    regime on shapes without jumps, both corners"""
    names = list(SHAPES)
    cases = []
    for i, S in enumerate(SS):
        for j in range(3):
            depth = DEPTHS[(i + j) % len(DEPTHS)]
            if depth == "resampled" and S < 9:
                depth = "beyond_far" if S > 1 else "uniform"
            cases.append((names[(3 * i + j) % len(names)], RS[(i + j) % len(RS)], S, depth, OPACITIES[(i + 2 * j) % len(OPACITIES)]))
    plain = [n for n in names if not SHAPES[n][0].endswith("scaffold")]
    k = 0
    for depth in DEPTHS:
        for op in OPACITIES:
            extra = (plain[k % len(plain)], 9, (65, 130, 63)[k % 3], depth, op)
            k += 1
            if extra not in cases:
                cases.append(extra)
    for extra in (("triplane_c16_222x128", 130, 200, "resampled", "mixed"), ("triplane_c16_222x32", 1, 1, "uniform", "mixed"),
                  ("triplane_c16_322x64_contract_mask_scaffold", 130, 130, "resampled", "mixed")):
        if extra not in cases:
            cases.append(extra)
    return cases


CASES = _table()


def case_id(c):
    return "-".join(str(v) for v in c)


def contract_of(c):
    return scene(c[0])["contract"] or c[3] == "beyond_far"


def split_samples(S, depth):
    """how the sample ops make ``S`` samples of a regime: (regular, beyond far) of ``ray_samples``, or (coarse, new) of the resampling"""
    if depth == "beyond_far":
        k = min(3, S - 1)
        return S - k, k
    if depth == "resampled":
        return S // 3, S - S // 3
    return S, 0


def peak_index(R, S_coarse):
    """the coarse sample that carries a ray's weight: an inner one, at a position that moves with the ray"""
    return 1 + (torch.arange(R) * 5 + S_coarse // 2) % (S_coarse - 2)


def peaked_weights(R, S_coarse):
    """one peak per ray (``peak_index``) on a floor of zeros: nearly every new sample lands in its bin"""
    w = torch.zeros(R, S_coarse)
    w[torch.arange(R), peak_index(R, S_coarse)] = 1.0
    return w


def peaked_depths(depths):
    """the coarse depths with the peak's two neighbours moved onto it -- three equal depths, as the sorted union of an earlier
    resampling holds them; still non-decreasing.  The peak's bin then has zero width: the new samples that land in it are equal, to the
    bit, and the deltas between them are zero."""
    R, S = depths.shape
    j = peak_index(R, S).to(depths.device)
    r = torch.arange(R, device=depths.device)
    out = depths.clone()
    out[r, j - 1] = out[r, j + 1] = depths[r, j]
    return out


def definition(sc, rays, depths, deltas, gain, contract, leaves=None):
    """``(ray_length, -log T, feature [R, 3], weights)`` of the definition in the dtype of ``depths``.  ``leaves``: dict with the
    differentiable ``grids`` / ``cgrids`` / ``params`` / ``enc`` to use in place of the scene's (autograd then reaches them)."""
    dt = depths.dtype
    lv = leaves or {}
    grids = lv.get("grids") or [g.to(dt) for g in sc["grids"]]
    cgrids = lv.get("cgrids") or (None if sc["cgrids"] is None else [g.to(dt) for g in sc["cgrids"]])
    params = lv["params"] if "params" in lv else sc["dec"].mlp_params.to(dt)
    enc = lv["enc"] if "enc" in lv else rays.encoding.to(dt)
    dec = lp.DecoderParams(params, sc["dec"].n_hidden_trunk, sc["dec"].n_hidden_opacity, sc["dec"].n_hidden_color, sc["dec"].color_chn)
    points = depths[..., None] * rays.directions.to(dt)[:, None] + rays.origins.to(dt)[:, None]
    opacity, color = O.eval_decoder(points, grids, rays.grid_idx, dec, enc, gain, mask_out_of_bounds_samples=sc["mask"],
                                    scaffold=None if sc["scaffold"] is None else sc["scaffold"].to(dt), color_grids=cgrids,
                                    contract_coords=contract)
    return CC.composite(opacity, color[..., :3], depths, deltas)


def gain_for(sc, rays, depths, deltas, contract, regime):
    """the gain of an opacity regime at these (fp32 or fp64) depths: module docstring"""
    if regime == "mixed":
        return 1.7
    with torch.no_grad():
        nlt = definition(sc, rays, depths.double(), deltas.double(), 1.0, contract)[1]
    med = float(nlt.median())
    if not med > 0.0:
        return 1.7
    return (0.05 if regime == "transparent" else 800.0) / med

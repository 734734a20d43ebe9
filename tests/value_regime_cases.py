"""Value regimes of the compositing arithmetic: the table, the transform and the ledger (tests/test_value_regimes_host.py checks them
without a GPU, tests/test_gpu_value_regimes.py runs every copy of the arithmetic in every regime).

Every scene of tests/synth.py comes from one recipe -- N(0, 1) grids, N(0, 0.1-0.3) parameters, gain <= 3 -- and so reaches one path of
``softplus_f`` / ``__expf`` / ``sigmoid_f`` / ``nlt_add`` (csrc/lp_device.h): softplus arguments below 5 (and below -4.159 in one 24-ray
case), colour pre-activations within +-8, -log T below 20 over the regular samples (``OLD_COVERAGE``, asserted by the host test).  A REGIME moves a built case elsewhere without
touching its grids, rays or hidden layers -- so every ReLU decision stays what it was:

    raw_o -> a_o * raw_o + b_o      (last layer of the opacity head)
    raw_c -> a_c * raw_c            (last layer of the colour head)
    gain                            (decouples the size of raw_o from the size of -log T: every regime stays well conditioned)

written into the flat ``mlp_params`` through the views of ``oracle.split_decoder``.  What a regime has to REACH is a list of named
predicates (the ledger) over the values the fp64 oracle records while it runs (``oracle.value_recorder``): ``raw_o``, ``raw_c``, -log T
after every sample.  The constants per (carrier, regime) were searched on the CPU until the predicates held; the predicates decide, not
the constants.

The thresholds restate device lines:
* -4.159 = log(2^-6): below it ``softplus_f`` takes its series (lp_device.h:436 ``e < 0.015625f``);
* 20: above it ``softplus_f`` / ``d_softplus_f`` are linear / 1 (lp_device.h:437, :469);
* 88.8 > log(FLT_MAX) = 88.72: ``__expf(x)`` is inf, ``log(1 + exp(x))`` would overflow without the linear branch;
* -103.3 < log(2^-149): ``__expf(x)`` is exactly 0 whatever the denormal mode (it flushes from -87.3);
* 17: ``sg * (1 - sg)`` is exactly 0 in fp32 above it (1 - sg < 2^-24); -88.8: ``rcp(1 + __expf(-x))`` sees inf;
* 87.4: ``__expf(-nlt)`` is 0 beyond it: the ray is opaque to the last bit.
"""
from __future__ import annotations

import copy
import dataclasses
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Tuple

import torch

import lightplane_amd as lp
from lightplane_amd import _lib
from oracle import lightplane_oracle as O
from tests import partial_grad_cases as T
from tests.synth import RendererCase

F64 = torch.float64
SERIES_BELOW = -4.159   # log(2^-6) = -4.1589
LINEAR_ABOVE = 20.0
EXP_OVERFLOWS = 88.8
EXP_IS_ZERO = -103.3
COLOUR_SATURATES = 17.0
T_IS_ZERO = 87.4

REGIMES = ("init", "surface", "extremes", "opaque_late")


@dataclass(frozen=True)
class Constants:
    """The transform of one (carrier, regime) pair.  ``gain`` / ``num_samples`` / ``seed`` None: the carrier's own (another seed only
    where the fp32 oracle takes the other branch of a ReLU near tie at the carrier's own: the pair would fail its precondition for a reason
    that is not the regime's)."""
    a_o: float = 1.0
    b_o: float = 0.0
    a_c: float = 1.0
    gain: Optional[float] = None
    num_samples: Optional[int] = None
    seed: Optional[int] = None


@dataclass
class Recorded:
    """What the fp64 oracle saw: raw_o [R, S] (before the noise), softplus_in [R, S] (after it), raw_c [R, S, color_chn], nlt [R, S + 1];
    ``seg_len``: samples per segment of a segmented backward (0: one sweep)."""
    raw_o: torch.Tensor
    softplus_in: torch.Tensor
    raw_c: torch.Tensor
    nlt: Optional[torch.Tensor]
    seg_len: int = 0

    @property
    def final(self):
        return self.nlt[:, -1]


# ---- the transform ---------------------------------------------------------------------------------------------------------------------
def transform_decoder(dec, k: Constants):
    """A copy of ``dec`` whose last opacity layer computes a_o * raw_o + b_o and whose last colour layer a_c * raw_c."""
    flat = dec.mlp_params.detach().clone()
    _, (wo, bo), (wc, bc) = O.split_decoder(flat, dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color)
    wo[-1].mul_(k.a_o)           # (views of ``flat``)
    bo[-1].mul_(k.a_o).add_(k.b_o)
    wc[-1].mul_(k.a_c)
    bc[-1].mul_(k.a_c)
    changed = not torch.equal(flat, dec.mlp_params)
    assert changed or (k.a_o, k.b_o, k.a_c) == (1.0, 0.0, 1.0), "the transform did not reach the flat parameter tensor"
    return lp.DecoderParams(flat, dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)


def apply_regime(d: dict, k: Constants) -> dict:
    """The built case ``d`` (RendererCase.build()) in another value regime: same grids, rays, scaffold and upstream gradients."""
    out = dict(d)
    out["decoder"] = transform_decoder(d["decoder"], k)
    if k.gain is not None:
        out["cfg"] = dict(d["cfg"], gain=float(k.gain))
    return out


def with_zero_spans(d: dict) -> dict:
    """Every fourth ray of ``d`` with ``far == near``: all its samples sit on one point and every interval length is 0."""
    out = dict(d)
    rays = copy.copy(d["rays"])
    rays.far = d["rays"].far.clone()
    rays.far[::4] = d["rays"].near[::4]
    out["rays"] = rays
    return out


def rays_as(rays, dtype):
    r = copy.copy(rays)
    for f in ("directions", "origins", "near", "far", "encoding"):
        setattr(r, f, getattr(r, f).to(dtype))
    return r


def oracle_forward(d: dict, dtype=F64, record=False):
    """The plain oracle's three outputs in ``dtype``; with ``record`` also what ``oracle.value_recorder`` saw."""
    dec = copy.copy(d["decoder"])
    dec.mlp_params = dec.mlp_params.to(dtype)
    cg = None if d["color_grids"] is None else [g.to(dtype) for g in d["color_grids"]]
    sc = None if d["scaffold"] is None else d["scaffold"].to(dtype)
    with torch.no_grad(), O.value_recorder() as rec:
        out = O.lightplane_renderer_naive(rays_as(d["rays"], dtype), [g.to(dtype) for g in d["grids"]], dec, scaffold=sc, color_grid=cg, **d["cfg"])
    if not record:
        return out
    cc = int(d["decoder"].color_chn)
    return out, Recorded(rec.raw_o, rec.softplus_in, rec.raw_c[..., :cc], rec.nlt)


def oracle_gradients(d: dict, dtype=F64):
    """(outputs, grad_mlp_params, grad_encoding, grad_grids, grad_color_grids) of the plain oracle in ``dtype``."""
    rays = rays_as(d["rays"], dtype)
    rays.encoding = rays.encoding.clone().requires_grad_(True)
    dec = copy.copy(d["decoder"])
    dec.mlp_params = dec.mlp_params.to(dtype).clone().requires_grad_(True)
    grids = [g.to(dtype).clone().requires_grad_(True) for g in d["grids"]]
    cg = None if d["color_grids"] is None else [g.to(dtype).clone().requires_grad_(True) for g in d["color_grids"]]
    sc = None if d["scaffold"] is None else d["scaffold"].to(dtype)
    out = O.lightplane_renderer_naive(rays, grids, dec, scaffold=sc, color_grid=cg, **d["cfg"])
    u = [x.to(dtype) for x in d["upstream"]]
    ((out[0] * u[0]).sum() + (out[1] * u[1]).sum() + (out[2] * u[2]).sum()).backward()
    return [o.detach() for o in out], dec.mlp_params.grad, rays.encoding.grad, [g.grad for g in grids], None if cg is None else [g.grad for g in cg]


# ---- the ledger: what a regime has to reach ------------------------------------------------------------------------------------------------
def _frac(mask) -> float:
    return float(mask.double().mean())


def init_every_raw_o_on_the_series_branch(r: Recorded):
    """lp_device.h:436: every raw_o in (-6, -4.159) -- ``e < 2^-6``, the series of log1p; where the module starts (modules.py: opacity_init_bias = -5)"""
    return bool(((r.raw_o > -6.0) & (r.raw_o < SERIES_BELOW)).all())


def init_every_ray_nearly_transparent(r: Recorded):
    """lp_renderer_generic.hip:80-81: final -log T of every ray in [1e-3, 1e-1] -- ``w = t_prev - t`` with both within 10 % of 1"""
    return bool(((r.final >= 1e-3) & (r.final <= 1e-1)).all())


def surface_quarter_on_the_series_branch(r: Recorded):
    """lp_device.h:436: raw_o < -4.159 for >= 25 % of the samples (empty space in front of a surface)"""
    return _frac(r.raw_o < SERIES_BELOW) >= 0.25


def surface_tenth_on_the_log_branch(r: Recorded):
    """lp_device.h:435: raw_o in (-4.159, 20] for >= 10 % of the samples (``__logf(1 + e)``)"""
    return _frac((r.raw_o > SERIES_BELOW) & (r.raw_o <= LINEAR_ABOVE)) >= 0.10


def surface_rays_go_opaque_within_two_samples(r: Recorded):
    """lp_renderer_generic.hip:80-81: >= 10 % of the rays go from T > 0.9 to T < 1e-3 within two samples (all of w on one or two samples)"""
    t = torch.exp(-r.nlt)
    return _frac(((t[:, :-2] > 0.9) & (t[:, 2:] < 1e-3)).any(dim=1)) >= 0.10


def surface_rays_end_with_t_exactly_zero(r: Recorded):
    """lp_renderer_generic.hip:80: >= 10 % of the rays end with -log T > 87.4 (``__expf(-nlt)`` is 0 and stays 0)"""
    return _frac(r.final > T_IS_ZERO) >= 0.10


def extremes_exp_overflows(r: Recorded):
    """lp_device.h:433, :437: raw_o > 88.8 for >= 1 % of the samples (``__expf(x)`` is inf: only the ``x > 20`` selection keeps it out)"""
    return _frac(r.raw_o > EXP_OVERFLOWS) >= 0.01


def extremes_exp_is_zero(r: Recorded):
    """lp_device.h:433, :467: raw_o < -103.3 for >= 1 % of the samples (``__expf(x)`` is 0; ``rcp(1 + __expf(-x))`` of d_softplus sees inf)"""
    return _frac(r.raw_o < EXP_IS_ZERO) >= 0.01


def extremes_linear_branch_without_overflow(r: Recorded):
    """lp_device.h:437, :469: raw_o in (20, 88.8] for >= 1 % of the samples"""
    return _frac((r.raw_o > LINEAR_ABOVE) & (r.raw_o <= EXP_OVERFLOWS)) >= 0.01


def extremes_colour_saturates(r: Recorded):
    """lp_device.h:467, lp_renderer_generic.hip:236: raw_c > 17 for >= 1 % of the colour entries (``sg * (1 - sg)`` is exactly 0)"""
    return _frac(r.raw_c > COLOUR_SATURATES) >= 0.01


def extremes_colour_rcp_of_inf(r: Recorded):
    """lp_device.h:467: raw_c < -88.8 for >= 1 % of the colour entries (``rcp(1 + inf)``)"""
    return _frac(r.raw_c < -EXP_OVERFLOWS) >= 0.01


def extremes_outputs_stay_informative(r: Recorded):
    """lp_renderer_generic.hip:75-81: final -log T in [0.05, 20] for >= 80 % of the rays"""
    return _frac((r.final >= 0.05) & (r.final <= 20.0)) >= 0.80


def opaque_late_large_final(r: Recorded):
    """lp_device.h:114 (nlt_add), lp_renderer_generic.hip:213: the largest final -log T is >= 1e3 (the backward subtracts from it)"""
    return float(r.final.max()) >= 1e3


def opaque_late_small_value_behind_a_large_checkpoint(r: Recorded):
    """lp_renderer_generic.hip:204-215, lp_renderer_mfma_bwd.h (re-anchor every LP_NLT_CKPT = 32 samples): >= 10 % of the rays have their
    first sample with T < 1e-3 at index >= 32 (segmented backward: in a segment other than the first) -- the backward reconstructs a small
    -log T by subtracting from a large checkpoint"""
    t = torch.exp(-r.nlt[:, 1:])
    opaque = t < 1e-3
    first = torch.where(opaque.any(dim=1), opaque.double().argmax(dim=1), torch.full((t.shape[0],), -1))
    return _frac(first >= (r.seg_len if r.seg_len else _lib.LP_NLT_CKPT)) >= 0.10


LEDGER: Dict[str, Tuple[Callable[[Recorded], bool], ...]] = {
    "init": (init_every_raw_o_on_the_series_branch, init_every_ray_nearly_transparent),
    "surface": (surface_quarter_on_the_series_branch, surface_tenth_on_the_log_branch, surface_rays_go_opaque_within_two_samples,
                surface_rays_end_with_t_exactly_zero),
    "extremes": (extremes_exp_overflows, extremes_exp_is_zero, extremes_linear_branch_without_overflow, extremes_colour_saturates,
                 extremes_colour_rcp_of_inf, extremes_outputs_stay_informative),
    "opaque_late": (opaque_late_large_final, opaque_late_small_value_behind_a_large_checkpoint),
}
# (evaluations at points and on the scaffold's lattice have no march: the predicates over -log T do not apply to them)
POINTWISE = {
    "init": (init_every_raw_o_on_the_series_branch,),
    "surface": (surface_quarter_on_the_series_branch, surface_tenth_on_the_log_branch),
    "extremes": (extremes_exp_overflows, extremes_exp_is_zero, extremes_linear_branch_without_overflow, extremes_colour_saturates,
                 extremes_colour_rcp_of_inf),
}


def missed(regime: str, r: Recorded, table=None) -> List[str]:
    return [p.__name__ for p in (table or LEDGER)[regime] if not p(r)]


def ranges(r: Recorded) -> dict:
    """the figures of the coverage table"""
    out = dict(raw_o=(float(r.raw_o.min()), float(r.raw_o.max())))
    if r.raw_c.numel():
        out["raw_c"] = (float(r.raw_c.min()), float(r.raw_c.max()))
    if r.nlt is not None:
        out["final_nlt"] = (float(r.final.min()), float(r.final.max()))
    return out


# what the recipe of tests/synth.py reaches over the unchanged RENDERER_CASES ("Value regimes"; asserted by the host test):
# softplus arguments in (-6.7, 5) and below -4.159 in one 24-ray case only, |raw_c| < 8, -log T < 20 over the regular samples
OLD_COVERAGE = dict(softplus_in_min=-6.7, softplus_in_max=5.0, raw_c_abs_max=8.0, regular_nlt_max=20.0,
                    series_branch_cases=("flex_121_h16_c32_noise",))


# ---- Renderer carriers: the 17 launches of tests/partial_grad_cases.py ----------------------------------------------------------------------
K = Constants
# searched on the CPU (quantiles of the carrier's own raw_o / raw_c mapped onto the thresholds, then a gain) until the predicates held
RENDERER_CONSTANTS: Dict[Tuple[str, str], Constants] = {
    ("tuned_tri_c16", "init"): K(a_o=0.05, b_o=-5.0),
    ("tuned_tri_c16", "surface"): K(a_o=25.0, gain=100.0),
    ("tuned_tri_c16", "extremes"): K(a_o=200.0, b_o=80.0, a_c=40.0, gain=0.02),
    ("tuned_tri_c16", "opaque_late"): K(a_o=45.0, gain=300.0, num_samples=70),
    ("tuned_vox_c32", "init"): K(a_o=0.05, b_o=-5.0),
    ("tuned_vox_c32", "surface"): K(a_o=25.0, b_o=-20.0, gain=10.0),
    ("tuned_vox_c32", "opaque_late"): K(a_o=45.0, b_o=-40.0, gain=30.0, num_samples=70),
    ("tuned_nonplain", "init"): K(a_o=0.05, b_o=-5.0, gain=1e-05),
    ("tuned_nonplain", "surface"): K(a_o=25.0, b_o=-5.0, gain=10.0),
    ("tuned_nonplain", "opaque_late"): K(a_o=45.0, gain=30.0, num_samples=70),
    ("tuned_seg", "init"): K(a_o=0.05, b_o=-5.0),
    ("tuned_seg", "surface"): K(a_o=25.0, b_o=-15.0, gain=10.0),
    ("tuned_seg", "extremes"): K(a_o=300.0, b_o=-40.0, a_c=40.0, gain=0.02),
    ("tuned_seg", "opaque_late"): K(a_o=45.0, b_o=-30.0, gain=30.0),
    ("tuned_nw8", "init"): K(a_o=0.05, b_o=-5.0, gain=3e-05),
    ("tuned_nw8", "surface"): K(a_o=15.0, gain=0.01),
    ("tuned_nw8", "opaque_late"): K(a_o=45.0, gain=30.0, num_samples=70),
    ("tuned_tm", "init"): K(a_o=0.05, b_o=-5.0),
    ("tuned_tm", "surface"): K(a_o=25.0, b_o=-10.0, gain=30.0),
    ("tuned_tm", "opaque_late"): K(a_o=45.0, b_o=-20.0, gain=300.0, num_samples=70),
    ("tuned_fp32", "init"): K(a_o=0.05, b_o=-5.0),
    ("tuned_fp32", "surface"): K(a_o=25.0, b_o=-10.0, gain=30.0),
    ("tuned_fp32", "extremes"): K(a_o=200.0, b_o=-40.0, a_c=40.0, gain=0.02),
    ("tuned_fp32", "opaque_late"): K(a_o=45.0, b_o=-10.0, gain=30.0, num_samples=70),
    ("loop_deep_424", "init"): K(a_o=0.05, b_o=-5.0),
    ("loop_deep_424", "surface"): K(a_o=25.0, b_o=-5.0, gain=300.0),
    ("loop_deep_424", "opaque_late"): K(a_o=90.0, b_o=-10.0, gain=300.0, num_samples=70),
    ("loop_shallow_h16", "init"): K(a_o=0.05, b_o=-5.0),
    ("loop_shallow_h16", "surface"): K(a_o=25.0, b_o=-5.0, gain=30.0),
    ("loop_shallow_h16", "extremes"): K(a_o=120.0, b_o=20.0, a_c=40.0, gain=0.02),
    ("loop_shallow_h16", "opaque_late"): K(a_o=45.0, gain=30.0, num_samples=70),
    ("loop_h64_two_block", "init"): K(a_o=0.05, b_o=-5.0, gain=3e-05),
    ("loop_h64_two_block", "surface"): K(a_o=25.0, b_o=-5.0, gain=10.0),
    ("loop_h64_two_block", "extremes"): K(a_o=200.0, b_o=20.0, a_c=80.0, gain=1e-06),
    ("loop_h64_two_block", "opaque_late"): K(a_o=45.0, gain=30.0, num_samples=70),
    ("loop_c64", "init"): K(a_o=0.05, b_o=-5.0),
    ("loop_c64", "surface"): K(a_o=40.0, gain=30.0),
    ("loop_c64", "opaque_late"): K(a_o=45.0, gain=300.0, num_samples=70),
    ("loop_seg", "init"): K(a_o=0.05, b_o=-5.0),
    ("loop_seg", "surface"): K(a_o=25.0, b_o=-5.0, gain=300.0),
    ("loop_seg", "opaque_late"): K(a_o=45.0, gain=60.0),
    ("loop_two_grid", "init"): K(a_o=0.05, b_o=-5.0),
    ("loop_two_grid", "surface"): K(a_o=25.0, gain=30.0),
    ("loop_two_grid", "extremes"): K(a_o=120.0, b_o=80.0, a_c=40.0, gain=0.02),
    ("loop_two_grid", "opaque_late"): K(a_o=45.0, gain=100.0, num_samples=70),
    ("loop_two_grid_h64", "init"): K(a_o=0.05, b_o=-5.0),
    ("loop_two_grid_h64", "surface"): K(a_o=25.0, b_o=-10.0, gain=30.0),
    ("loop_two_grid_h64", "extremes"): K(a_o=120.0, a_c=40.0, gain=0.02),
    ("loop_two_grid_h64", "opaque_late"): K(a_o=45.0, gain=30.0, num_samples=70),
    ("generic_lds", "init"): K(a_o=0.05, b_o=-5.0),
    ("generic_lds", "surface"): K(a_o=15.0, b_o=-20.0, gain=30.0),
    ("generic_lds", "opaque_late"): K(a_o=30.0, b_o=-30.0, gain=30.0, num_samples=70),
    ("generic_global", "init"): K(a_o=0.05, b_o=-5.0),
    ("flat_grid", "init"): K(a_o=0.05, b_o=-5.0),
    ("flat_grid", "surface"): K(a_o=25.0, b_o=-10.0, gain=10.0),
    ("flat_grid", "opaque_late"): K(a_o=45.0, b_o=-30.0, gain=100.0, num_samples=70, seed=102),   # (seed 2 at 70 samples: an fp32 ReLU tie)
    ("tuned_vox_c32", "extremes"): K(a_o=307.0, b_o=-228.0, a_c=48.1, gain=0.02),
    ("tuned_nonplain", "extremes"): K(a_o=392.0, b_o=123.0, a_c=53.5, gain=1e-07),
    ("tuned_nw8", "extremes"): K(a_o=568.0, b_o=245.0, a_c=51.3, gain=3e-07),
    ("tuned_tm", "extremes"): K(a_o=292.0, b_o=-89.9, a_c=35.3, gain=0.02),
    ("loop_deep_424", "extremes"): K(a_o=1030.0, b_o=-71.2, a_c=55.0, gain=0.02),
    ("loop_c64", "extremes"): K(a_o=547.0, b_o=42.7, a_c=107.0, gain=0.02),
    ("loop_seg", "extremes"): K(a_o=713.0, b_o=-24.2, a_c=43.7, gain=0.02),
    ("generic_lds", "extremes"): K(a_o=131.0, b_o=-177.0, a_c=40.5, gain=0.1),
    ("generic_global", "surface"): K(a_o=484.0, b_o=-19.3, gain=10.0),
    ("generic_global", "extremes"): K(a_o=2770.0, b_o=-110.0, a_c=186.0, gain=0.02),
    ("generic_global", "opaque_late"): K(a_o=647.0, b_o=-30.5, gain=30.0, num_samples=70),
    ("flat_grid", "extremes"): K(a_o=160.0, b_o=-96.0, a_c=50.0, gain=0.02),
}

# ``init`` on a carrier with beyond-far samples: the last interval is far / disparity_at_inf = 3e5 long, so a final -log T below 0.1 needs a
# gain of 3e-5, and the regular samples' ``w = T_{i-1} - T_i`` falls below one ulp of T = 1 -- the cancellation of the reference's own
# formula.  The fp32 oracle's grid gradient is 6e-5 off the fp64 oracle's there (every output still within 2e-5); not reseeded away.
CANCELLATION_PAIRS = (("loop_h64_two_block", "init"),)
ZERO_SPAN_ENTRIES = ("tuned_tri_c16", "loop_deep_424", "generic_lds")   # one tuned, one looped, one shape-generic
RENDERER_PAIRS = [(e.id, r) for e in T.RENDERER_ENTRIES for r in REGIMES]
_BUILT = {}


def renderer_entry(entry_id: str, regime: str) -> T.RendererEntry:
    """The entry of tests/partial_grad_cases.py with the regime's sample count (every other field unchanged)."""
    e = T.renderer_entry(entry_id)
    k = RENDERER_CONSTANTS[(entry_id, regime)] if regime != "zero_span" else Constants()
    if k.num_samples is not None:
        e = dataclasses.replace(e, case=dataclasses.replace(e.case, num_samples=k.num_samples))
    if k.seed is not None:
        e = dataclasses.replace(e, case=dataclasses.replace(e.case, seed=k.seed))
    return e


def built_renderer(entry_id: str, regime: str):
    """(entry, inputs) of a (carrier, regime) pair -- ``regime`` "zero_span": the unchanged case with every fourth ray's far == near.
    Built once per process and never modified."""
    key = (entry_id, regime)
    if key not in _BUILT:
        e = renderer_entry(entry_id, regime)
        d = e.case.build()
        d = with_zero_spans(d) if regime == "zero_span" else apply_regime(d, RENDERER_CONSTANTS[key])
        _BUILT[key] = (e, d)
    return _BUILT[key]


def recorded_renderer(e: T.RendererEntry, d: dict):
    """(fp64 outputs, Recorded) of a Renderer carrier; ``seg_len`` set for a segmented backward"""
    out, r = oracle_forward(d, F64, record=True)
    r.seg_len = _lib.LP_SEG_LEN if e.segments > 1 else 0
    return out, r


# ---- deep forward: family 3 (resident weight images) and family 4 (streamed) forward, shape-generic backward -----------------------------------
POINT_REGIMES = ("init", "surface", "extremes")
_DEEP = dict(T.NO_SEG, deep_forward_mfma=True)
DEEP_ENTRIES = [
    T.RendererEntry("deep_resident_322", "forward of a 3/2/2 x 64 decoder on resident weight images (lp_renderer_loop.h), shape-generic backward",
                    RendererCase("deep_resident_322", seed=61, n_rays=T.N_RAYS, grid_base=(2, 6, 7, 5, 16), is_triplane=True, n_layers=(3, 2, 2),
                                 hidden=64, num_samples=21), config=_DEEP, family=0),
    T.RendererEntry("deep_streamed_444", "forward of a 4/4/4 x 64 decoder on streamed weight images (lp_renderer_loop_stream.hip), shape-generic backward",
                    RendererCase("deep_streamed_444", seed=62, n_rays=T.N_RAYS, grid_base=(2, 5, 6, 7, 32), n_layers=(4, 4, 4), hidden=64,
                                 num_samples=21), config=_DEEP, family=0),
]
DEEP_FORWARD_FAMILY = {"deep_resident_322": 3, "deep_streamed_444": 4}
DEEP_CONSTANTS: Dict[Tuple[str, str], Constants] = {
    ("deep_resident_322", "init"): K(a_o=0.05, b_o=-5.0),
    ("deep_resident_322", "surface"): K(a_o=10.4, b_o=-8.75, gain=10.0),
    ("deep_resident_322", "extremes"): K(a_o=82.5, b_o=-95.9, a_c=23.0, gain=0.05),
    ("deep_streamed_444", "init"): K(a_o=0.05, b_o=-5.0),
    ("deep_streamed_444", "surface"): K(a_o=12.8, b_o=0.558, gain=10.0),
    ("deep_streamed_444", "extremes"): K(a_o=65.7, b_o=18.0, a_c=44.2, gain=0.02),
}
DEEP_PAIRS = [(e.id, r) for e in DEEP_ENTRIES for r in POINT_REGIMES]


def built_deep(entry_id: str, regime: str):
    key = (entry_id, regime)
    if key not in _BUILT:
        e = next(x for x in DEEP_ENTRIES if x.id == entry_id)
        _BUILT[key] = (e, apply_regime(e.case.build(), DEEP_CONSTANTS[key]))
    return _BUILT[key]


# ---- evaluation at points (lp_points.hip) and on the scaffold's lattice (lp_scaffold.hip): no march, gain as the case has it --------------------
POINTS_CONSTANTS: Dict[Tuple[str, str], Constants] = {   # (He-initialised decoders: raw_o spans [-2, 2] before the transform)
    ("triplane_c16_222x32", "init"): K(a_o=0.508, b_o=-4.63),
    ("triplane_c16_222x32", "surface"): K(a_o=30.0, b_o=17.4),
    ("triplane_c16_222x32", "extremes"): K(a_o=176.0, b_o=106.0, a_c=42.0),
    ("voxel_c32_112x64_flat", "init"): K(a_o=1.07, b_o=-5.17),
    ("voxel_c32_112x64_flat", "surface"): K(a_o=62.1, b_o=-8.13),
    ("voxel_c32_112x64_flat", "extremes"): K(a_o=402.0, b_o=-57.9, a_c=44.7),
}
POINTS_PAIRS = list(POINTS_CONSTANTS)


def points_case(name: str, regime: str):
    """tests/points_cases.py::case(name) with the regime's decoder: the same points, masks and zeroed upstream gradients"""
    from tests import points_cases as PC
    k = POINTS_CONSTANTS[(name, regime)]
    assert k.gain is None and k.num_samples is None
    return PC.case(name, decoder_transform=lambda dec: transform_decoder(dec, k), key=(name, regime))


SCAFFOLD_CASE = "triplane_c16_22x32_r1"
SCAFFOLD_CONSTANTS: Dict[str, Constants] = {
    "init": K(a_o=0.761, b_o=-4.39),
    "extremes": K(a_o=303.0, b_o=232.0),
}
SCAFFOLD_POINTWISE = {
    "init": (init_every_raw_o_on_the_series_branch,),
    "extremes": (extremes_exp_overflows, extremes_exp_is_zero, extremes_linear_branch_without_overflow),
}


def scaffold_case(regime: str):
    """The case of tests/test_gpu_scaffold.py with the regime's decoder: dict(size, grids, dec, op (fp64 ``gain * softplus``), mask, form,
    seen (Recorded over every lattice point of every batch element))."""
    key = ("scaffold", regime)
    if key not in _BUILT:
        from tests import test_gpu_scaffold as S
        c = S._case(SCAFFOLD_CASE)
        dec = transform_decoder(c["dec"], SCAFFOLD_CONSTANTS[regime])
        B, D, H, W = c["size"]
        d64 = lp.DecoderParams(dec.mlp_params.double(), dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
        enc = torch.zeros(1, int(dec.n_hidden_color[0]), dtype=F64)
        ops, raws = [], []
        for b in range(B):
            with torch.no_grad(), O.value_recorder() as seen:
                op = O.eval_decoder(S._lattice(D, H, W).double(), [g.double() for g in c["grids"]], torch.tensor([b]), d64, enc, S.GAIN,
                                    mask_out_of_bounds_samples=c["mask"])[0]
            ops.append(op.reshape(D, H, W))
            raws.append(seen.raw_o)
        raw = torch.cat(raws)
        _BUILT[key] = dict(size=c["size"], grids=c["grids"], dec=dec, op=torch.stack(ops), mask=c["mask"], form=c["form"], gain=S.GAIN,
                           seen=Recorded(raw, raw, torch.zeros(0), None))
    return _BUILT[key]

"""Scripted ray batches for early ray termination (``stop_transmittance``) and the stop indices the fp64 oracle expects of them
(tests/test_early_stop_host.py checks the table without a GPU, tests/test_gpu_early_stop.py holds every kernel family to it).

The march rule (``oracle.early_stop_index``): consecutive rays form groups -- one wavefront's rays: 32 in the tuned and the layer-looped
family, 64 in the shape-generic kernels -- and a group stops behind the first sample at which EVERY ray of it has -log T >= -log(eps).
A dense random scene stops every group at about the same small sample.  Here a SCRIPT says where each group stops:

* ``Group(target)``: the group's rays keep their origins, directions and ``near``; their span ``far - near`` is scaled by one factor per
  group.  Per-sample -log T scales with ``(far - near) / (S - 1)``, so the factor moves the stop through the march; it is SOLVED with
  the fp64 oracle: of a ladder of factors the one whose group stops at ``target`` with the largest decisive margins.  ``target=None``:
  a group that never stops.
* ``Group(target, held=k)``: only ``k`` rays in the middle of the group are solved; the others take ``FAST_SPAN`` and are opaque many
  times over (-log T > 80) when the ``k`` transparent ones let the group go.
* ``pool=True`` (the scaffold case): nothing is scaled.  The scaffold empties the half-space x < 0; the groups are PICKED from a pool of
  random rays by the sample at which each ray alone is through -- rays that see only empty space never stop (-log T exactly 0).

What a builder returns as expected is ``early_stop_index`` of the final batch, not the script's intent, and with it the two decisive
margins per group.  THE TIE CONDITION (asserted by the host test): both margins of every group are at least ``10 x 1e-4 x`` the largest
-log T the truncated march returns -- 1e-4 of a tensor's largest entry is the suite's bar on every output, so a kernel that meets the bar
on -log T is ten times too close to the oracle to land on the other side of the threshold.  The GPU test may then demand EQUAL indices.
"""
from __future__ import annotations

import copy
import functools
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from lightplane_amd import _lib
from oracle import lightplane_oracle as O
from tests.synth import RendererCase
from tests.value_regime_cases import rays_as

F64 = torch.float64
S = 40                     # regular samples: indices 31 and 32 lie on either side of the first -log T checkpoint (LP_NLT_CKPT = 32)
N_RAYS = 300               # two full 128-ray workgroups of the tuned family + a 32-ray wave + a 12-ray wave
TIE_FACTOR = 10.0
OUTPUT_BAR = 1e-4          # the suite's bar on every output, relative to the tensor's largest entry
FAST_SPAN = 6.0            # span factor of the opaque rays of a held-back group
LADDER = torch.logspace(math.log10(0.01), math.log10(40.0), 40, dtype=F64)   # span factors that bracket every group's
REFINE = 32                # rungs of the second pass, inside each group's bracket
MARGIN_CAP = 0.2           # a margin above this fraction of the threshold is as good as any (keeps -log T, and with it the bar, small)


@dataclass(frozen=True)
class Group:
    target: Optional[int]   # last sample the group marches; None: it never stops
    held: int = 0           # > 0: only this many rays (in the middle of the group) are solved, the others take FAST_SPAN


@dataclass(frozen=True)
class Case:
    name: str
    seed: int
    groups: Tuple[Group, ...]
    group: int = 32                         # rays per voting wavefront of the kernel that runs the case
    workgroup: int = 128                    # rays per workgroup of its backward (the sample loop starts at the workgroup's largest index)
    kernel: int = _lib.LP_KERNEL_AUTO
    family: int = 1                         # lp_renderer_kernel_family of the shapes (0 with LP_KERNEL_GENERIC)
    grid_base: tuple = (1, 10, 10, 10, 16)
    is_triplane: bool = False
    n_layers: tuple = (2, 2, 2)
    hidden: int = 32
    separate_color_grid: bool = False
    num_samples_inf: int = 0
    contract: bool = False
    mask_oob: bool = False
    noise_sigma: float = 0.0
    gain: float = 40.0
    eps: float = 1e-5
    param_std: float = 0.2
    pool: bool = False                      # pick the groups from a pool of rays behind a half-empty scaffold instead of scaling spans
    n_rays: int = N_RAYS

    @property
    def s_tot(self):
        return S + self.num_samples_inf

    @property
    def stop_neg_log_t(self):
        return -math.log(self.eps)


def _g(*targets):
    return tuple(t if isinstance(t, Group) else Group(t) for t in targets)


# 32-ray groups: workgroup 0 = groups 0-3, workgroup 1 = groups 4-7, workgroup 2 = group 8 and the 12-ray group 9.  Ray 0 -- the ray
# whose data an out-of-range lane of the last wave loads -- sits in a group that never stops: a vote of those lanes would hold the 12-ray
# group back to the last sample.
_G32 = _g(None, 0, 31, 32, 12, 33, 20, 5, 26, 17)
_G32_INF = _g(42, 20, 43, 31, 32, 41, 0, 45, 38, 40)
_G32_EARLY = _g(None, Group(14, held=1), 6, 9, 2, 11, 4, 8, 7, 10)
_G64 = _g(None, 0, 31, 32, 20)            # 64-ray groups: four full ones and one of 44 rays

CASES = (
    Case("tuned_c16_voxel", 1, _G32),
    Case("tuned_c32_triplane_inf8", 2, _G32_INF, grid_base=(1, 12, 12, 12, 32), is_triplane=True, num_samples_inf=8, contract=True, eps=1e-4),
    Case("tuned_c16_noise_contract_mask", 3, _g(None, 3, 32, 31, 16, 9, 35, 24, 1, 28), grid_base=(1, 8, 8, 8, 16), noise_sigma=0.5, contract=True,
         mask_oob=True, eps=1e-4),
    Case("tuned_c32_held_back", 4, _G32_EARLY, grid_base=(1, 8, 8, 8, 32)),
    Case("tuned_c16_scaffold_pool", 5, _g(None, 6, 30, 12, 18, None, 9, 24, 15, 21), grid_base=(1, 8, 8, 8, 16), pool=True, gain=25.0),
    Case("colour_grid_c16", 6, _G32, family=3, grid_base=(1, 9, 9, 9, 16), n_layers=(0, 2, 2), separate_color_grid=True),
    Case("looped_shallow_112_h64", 7, _G32, family=3, grid_base=(1, 8, 8, 8, 32), n_layers=(1, 1, 2), hidden=64, param_std=0.15),
    Case("looped_deep_333_h32_inf8", 8, _G32_INF, family=3, grid_base=(1, 10, 10, 10, 16), is_triplane=True, n_layers=(3, 3, 3), num_samples_inf=8,
         contract=True),
    Case("generic_64", 9, _G64, group=64, workgroup=64, kernel=_lib.LP_KERNEL_GENERIC, family=0, grid_base=(1, 8, 8, 8, 16)),
    Case("generic_64_h64_deep_inf8", 10, _g(42, 44, 31, 32, 41), group=64, workgroup=64, kernel=_lib.LP_KERNEL_GENERIC, family=0,
         grid_base=(1, 8, 8, 8, 32), n_layers=(3, 2, 2), hidden=64, num_samples_inf=8, contract=True, param_std=0.15, eps=1e-4),
)
CASE_IDS = [c.name for c in CASES]


# ---- the fp64 oracle's -log T along every ray -------------------------------------------------------------------------------------------------
def neg_log_t_cum(d: dict, last_sample=None) -> torch.Tensor:
    """-log T behind every sample, ``[R, S_tot]`` in fp64, of the built case ``d`` (the full march unless ``last_sample`` is given)."""
    dec = copy.copy(d["decoder"])
    dec.mlp_params = dec.mlp_params.to(F64)
    cg = None if d["color_grids"] is None else [g.to(F64) for g in d["color_grids"]]
    sc = None if d["scaffold"] is None else d["scaffold"].to(F64)
    with torch.no_grad(), O.value_recorder() as rec:
        O.lightplane_renderer_naive(rays_as(d["rays"], F64), [g.to(F64) for g in d["grids"]], dec, scaffold=sc, color_grid=cg,
                                    last_sample=last_sample, **d["cfg"])
    return rec.nlt[:, 1:]


def _with_far(d: dict, far: torch.Tensor) -> dict:
    out = dict(d)
    out["rays"] = copy.copy(d["rays"])
    out["rays"].far = far.to(torch.float32)
    return out


def _score(st: O.EarlyStop, thr: float) -> float:
    return min(float(st.margin_reached[0]), float(st.margin_before[0]), MARGIN_CAP * thr)


def _solve_spans(case: Case, d: dict) -> dict:
    """Per group the span factor that puts its stop at the scripted sample with the largest (capped) margins; of equally good ones the
    smallest.  Two passes, each one oracle march of the whole batch per rung (a ray's -log T does not depend on the other rays; the
    injected noise depends on the ray's index, which stays): the coarse LADDER brackets every group's factor, a ladder of REFINE rungs of
    the group's own inside its bracket settles it."""
    near, span = d["rays"].near.to(F64), (d["rays"].far - d["rays"].near).to(F64)
    thr = case.stop_neg_log_t
    bounds = [(g * case.group, min((g + 1) * case.group, case.n_rays)) for g in range(len(case.groups))]
    solved = torch.ones(case.n_rays, dtype=torch.bool)
    for (lo, hi), spec in zip(bounds, case.groups):
        if spec.held:
            solved[lo:hi] = False
            mid = lo + (hi - lo) // 2
            solved[mid:mid + spec.held] = True

    def march(factor):   # [R] span factors of the solved rays -> -log T [R, S_tot]
        return neg_log_t_cum(_with_far(d, near + torch.where(solved, factor, torch.full_like(factor, FAST_SPAN)) * span))

    def stop_of(nlt, g):
        lo, hi = bounds[g]
        return O.early_stop_index(nlt[lo:hi], thr, hi - lo)

    coarse = [march(torch.full((case.n_rays,), float(m), dtype=F64)) for m in LADDER]
    refine = torch.ones(len(case.groups), REFINE, dtype=F64)
    for g, spec in enumerate(case.groups):
        if spec.target is None:
            # a group that stays clear of the threshold but is no empty space: its slowest ray ends about half-way there
            lo, hi = bounds[g]
            k = min(range(len(LADDER)), key=lambda k: abs(float(coarse[k][lo:hi, -1].min()) / thr - 0.5))
            refine[g] = LADDER[k]
            continue
        idx = [int(stop_of(nlt, g).index[0]) for nlt in coarse]
        later = [k for k in range(len(LADDER)) if idx[k] > spec.target]        # smaller factors: the group stops later
        sooner = [k for k in range(len(LADDER)) if idx[k] < spec.target]
        m_lo = float(LADDER[max(later)]) if later else float(LADDER[0])
        m_hi = float(LADDER[min(sooner)]) if sooner else float(LADDER[-1])
        assert m_lo < m_hi, f"{case.name}: group {g}'s stop does not move through sample {spec.target} along the ladder"
        refine[g] = torch.logspace(math.log10(m_lo), math.log10(m_hi), REFINE, dtype=F64)
    of_ray = torch.arange(case.n_rays) // case.group
    fine = [march(refine[of_ray, j]) for j in range(REFINE)]
    factor = torch.ones(case.n_rays, dtype=F64)
    for g, spec in enumerate(case.groups):
        best, best_j = -1.0, None
        for j in range(REFINE if spec.target is not None else 1):
            st = stop_of(fine[j], g)
            if spec.target is None:
                assert float(st.margin_before[0]) > 0, f"{case.name}: group {g} was to stay clear of the threshold"
                best_j = j
            elif int(st.index[0]) == spec.target and _score(st, thr) > best + 1e-12:
                best, best_j = _score(st, thr), j
        assert best_j is not None, f"{case.name}: no span factor stops group {g} at sample {spec.target}"
        lo, hi = bounds[g]
        factor[lo:hi] = refine[g, best_j]
    return _with_far(d, near + torch.where(solved, factor, torch.full_like(factor, FAST_SPAN)) * span)


def _pick_from_pool(case: Case, d: dict) -> dict:
    """The scaffold case: ``d`` holds a pool of rays; every group is picked from it by the sample at which each ray ALONE is through.  One
    decisive ray -- through exactly at the scripted sample, with the largest margins the pool offers -- and rays that are through earlier
    and clear of the threshold by then; a group that never stops takes rays that see empty space only, or too little of the medium."""
    thr = case.stop_neg_log_t
    nlt = neg_log_t_cum(d)
    solo = O.early_stop_index(nlt, thr, 1)
    free = torch.ones(nlt.shape[0], dtype=torch.bool)
    picked = []
    for g, spec in enumerate(case.groups):
        n = min((g + 1) * case.group, case.n_rays) - g * case.group
        if spec.target is None:
            ok = free & (nlt[:, -1] < 0.5 * thr)
            empty = (ok & (nlt[:, -1] == 0)).nonzero()[:, 0]
            thin = (ok & (nlt[:, -1] > 0)).nonzero()[:, 0]
            ids = torch.cat([empty[:n // 2], thin[:n - min(n // 2, len(empty))]])
        else:
            t = spec.target
            score = torch.minimum(solo.margin_reached, solo.margin_before).clamp(max=MARGIN_CAP * thr)
            cand = (free & (solo.index == t)).nonzero()[:, 0]
            assert len(cand), f"{case.name}: no ray of the pool is through exactly at sample {t}"
            lead = cand[score[cand].argmax()]
            rest = free & (solo.index <= t) & (nlt[:, t] - thr >= score[lead])
            rest[lead] = False
            rest = rest.nonzero()[:, 0]
            # the decisive ray in the middle of the group, the others in pool order
            ids = torch.cat([rest[:n // 2], lead[None], rest[n // 2:n - 1]])
        assert len(ids) == n, f"{case.name}: the pool has {len(ids)} of the {n} rays group {g} needs"
        free[ids] = False
        picked.append(ids)
    idx = torch.cat(picked)
    out = dict(d)
    out["rays"] = d["rays"][idx]
    out["upstream"] = tuple(u[idx] for u in d["upstream"])
    return out


POOL_RAYS = 2400


@functools.lru_cache(maxsize=None)
def build(case: Case) -> dict:
    """``RendererCase.build()``'s dictionary for the scripted batch, plus ``stop_transmittance``, ``kernel``, ``group``, the fp64
    oracle's ``expected`` (``oracle.EarlyStop`` of the final batch), ``last_sample`` [R] (the expected index of every ray's group), the
    truncated march's ``max_neg_log_t`` and the ``tie_bar`` both margins of every group have to clear.  Cached: the GPU tests share it and
    leave it unchanged."""
    rc = RendererCase(case.name, seed=1000 + case.seed, n_rays=POOL_RAYS if case.pool else case.n_rays, grid_base=case.grid_base,
                      is_triplane=case.is_triplane, n_layers=case.n_layers, hidden=case.hidden, separate_color_grid=case.separate_color_grid,
                      num_samples=S, num_samples_inf=case.num_samples_inf, gain=case.gain, mask_oob=case.mask_oob, contract=case.contract,
                      noise_sigma=case.noise_sigma, noise_seed=77 + case.seed, param_std=case.param_std)
    d = rc.build()
    if case.pool:
        d["scaffold"] = torch.ones(1, 4, 4, 4)
        d["scaffold"][..., :2] = 0.0          # x < 0: empty space
        d = _pick_from_pool(case, d)
    else:
        d = _solve_spans(case, d)
    thr = case.stop_neg_log_t
    nlt = neg_log_t_cum(d)
    expected = O.early_stop_index(nlt, thr, case.group)
    last = expected.index.repeat_interleave(case.group)[:case.n_rays]
    returned = nlt.gather(1, last[:, None])[:, 0]        # -log T the truncated march returns
    d.update(stop_transmittance=case.eps, kernel=case.kernel, group=case.group, expected=expected, last_sample=last, neg_log_t_full=nlt,
             max_neg_log_t=float(returned.max()), tie_bar=TIE_FACTOR * OUTPUT_BAR * float(returned.max()))
    return d


def expected_flags(case: Case, last_sample: torch.Tensor) -> torch.Tensor:
    """The flag word of the DUMP twins per (ray, sample) that follows from the groups' indices: 1 up to the ray's own index, 2 from there
    to the largest index of its workgroup (the backward's sample loop is workgroup-uniform: a wave sits out the samples only a sibling
    wave marched), 0 behind it."""
    s = torch.arange(case.s_tot)[None, :]
    wg_last = torch.cat([last_sample[lo:lo + case.workgroup].max().expand(min(case.workgroup, case.n_rays - lo))
                         for lo in range(0, case.n_rays, case.workgroup)])
    own = s <= last_sample[:, None]
    return torch.where(own, 1, torch.where(s <= wg_last[:, None], 2, 0))

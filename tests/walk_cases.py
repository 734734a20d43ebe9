"""Scripted ray batches for the run-merged scatter walks and the ledger of the transitions they take (tests/test_walk_transitions_host.py
checks both without a GPU, tests/test_gpu_walk_transitions.py runs every user of the walks on them).

The walks -- the two forward kernels of csrc/lp_splatter.hip, ``splat_walk`` (the per-slot loop ``splat_walk_slots`` and
``splat_walk_unit_weights``) / ``splat_walk_vox`` / ``splat_walk_vox_feat2`` / ``splat_walk_vox_weights`` of
csrc/lp_splat_walk.h, their mirror ``splat_bwd_walk_kernel`` -- decide what a wave does by how a lane's cell lies to its predecessor's.
A pinhole image or a batch of random rays reaches those decisions by chance; here a SCRIPT says which cell every lane of a wave sits in:

* ``march_order="rays"`` (lane = ray): a ``Wave`` is 32 lanes ``(ix, iy, iz, entry)`` plus one step per sample common to the wave, in whole
  cells, so the pattern of sample 0 moves through the grid unchanged.  Ray r is the segment from its point at sample 0 to its point at
  sample S - 1: origin the first point, unit direction, near = 0, far = the length.
* ``march_order="samples"`` (lane = sample): a ``RayScript`` is the ray itself -- start and sample spacing in cells.

Cell coordinates are the Splatter's, ``t = (c + 1) / 2 * size - 0.5``; fractional parts lie in [0.3, 0.7] per axis (explicit ones where
a script wants a point out of bounds, 1 / 8 steps where a ray dwells), so no tap weight is small enough to hide behind the bar and the fp32
and fp64 geometries agree on every cell; encodings are per ray in [0.5, 1].

The LEDGER is a plain numpy model of who shares a wave with whom -- 32 rays per wave at C = 16 / 32 and 16 at C = 64, one ray x 32
samples in the transposed march, 8 rays per wave in the backward with ``patch_ray_index`` restated -- and of the walks' decisions
(run heads, axis election, carry conditions, the weight window), restated from the device code line by line.  From the oracle's fp32
geometry it forms every (wave, sample) lane sequence of (entry, ix, iy, iz, validity bits, live) and counts named PREDICATES; the
predicates decide what a case covers, not the script's intent.
"""
from __future__ import annotations

import copy
from collections import Counter
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from lightplane_amd import Rays
from oracle import lightplane_oracle as O

F64 = torch.float64
AXES = "xyz"
M0 = (0x55, 0x33, 0x0F)      # tap slots with the x / y / z bit clear (slot k = ux + 2 uy + 4 uz)
PACK_MAX = 1022              # lp_splat_walk.h: ``packable`` -- the 10-bit cell code holds index + 1 <= 1023


# ---- scripts ----------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Wave:
    """32 lanes (the last wave of a case may hold fewer): ``(ix, iy, iz, entry)`` or ``(ix, iy, iz, entry, (fx, fy, fz))`` with explicit
    fractional parts (None: drawn); ``step``: whole cells per sample, common to the wave."""
    lanes: tuple
    step: Tuple[int, int, int] = (0, 0, 1)


@dataclass(frozen=True)
class RayScript:
    start: Tuple[float, float, float]   # cell coordinates (x, y, z) of sample 0
    step: Tuple[float, float, float]    # cells per sample
    entry: int = 0


@dataclass(frozen=True)
class Case:
    name: str
    base: Tuple[int, int, int, int]     # (B, D, H, W) of the voxel grid the script is written for
    num_samples: int
    mask: bool
    waves: tuple = ()                   # march_order="rays"
    rays: tuple = ()                    # march_order="samples"
    row_length: int = 0                 # backward only: rays per image row
    seed: int = 0
    # the long-axis cases: first points and segments on the 2^-14 lattice of normalised coordinates, marched along an axis, with depths that
    # are dyadic -- every sample point and its cell coordinate (c + 1) * 750 - 0.5 is then EXACT in fp32.  Without it fp32 resolves a
    # coordinate of 1 500 cells to 1.2e-4 of a cell, which both the fp32 oracle and the kernels carry into every weight out there: measured
    # 2.1e-5 .. 3.5e-5 of the largest entry between the two oracles, above the 2e-5 they have to agree to -- the geometry's error, not a walk's.
    snap: bool = False

    @property
    def order(self):
        return "samples" if self.rays else "rays"


def rep(cell, n, b=0, frac=None):
    return ((cell[0], cell[1], cell[2], b) + ((frac,) if frac is not None else ()),) * n


def path(start, deltas, n, b=0):
    """lanes of n per cell along start, start + deltas[0], ..."""
    out, c = list(rep(start, n, b)), list(start)
    for d in deltas:
        c = [c[0] + d[0], c[1] + d[1], c[2] + d[2]]
        out += rep(tuple(c), n, b)
    return tuple(out)


def grid_sizes(case: Case, C: int, form: str = "voxel"):
    """The output grid-list of a case: "voxel", "voxel+xy" (the voxel grid and an xy plane: the one-axis walk and the plane walk in one
    launch) or "triplane" (three planes of the same axis sizes)."""
    B, D, H, W = case.base
    if form == "voxel":
        return [[B, D, H, W, C]]
    if form == "voxel+xy":
        return [[B, D, H, W, C], [B, 1, H, W, C]]
    assert form == "triplane"
    return [[B, 1, H, W, C], [B, D, 1, W, C], [B, D, H, 1, C]]


def _default_frac(gen, idx, size):
    """[0.3, 0.7]; in a border cell the half that lies inside [-1, 1] (a point out of bounds is a scripted decision, not a draw)"""
    u = float(torch.rand(1, generator=gen, dtype=F64))
    if idx == -1:
        return 0.55 + 0.15 * u
    if idx == size - 1:
        return 0.3 + 0.15 * u
    return 0.3 + 0.4 * u


def _coord(t, size):
    return (t + 0.5) * 2.0 / size - 1.0


_BUILT: Dict[Tuple[str, int], Rays] = {}


def build_rays(case: Case, C: int) -> Rays:
    """The fp32 ray batch of a case with ``C`` encoding channels.  Built once per process and never modified."""
    key = (case.name, C)
    if key in _BUILT:
        return _BUILT[key]
    B, D, H, W = case.base
    size = (W, H, D)
    gen = torch.Generator().manual_seed(1234 + case.seed)
    S = case.num_samples
    t0, t1, entry = [], [], []
    if case.order == "rays":
        for wi, wv in enumerate(case.waves):
            assert len(wv.lanes) == 32 or wi == len(case.waves) - 1, f"{case.name}: wave {wi} has {len(wv.lanes)} lanes"
            for ln in wv.lanes:
                fr = ln[4] if len(ln) > 4 else (None, None, None)
                a = [ln[k] + (fr[k] if fr[k] is not None else _default_frac(gen, ln[k], size[k])) for k in range(3)]
                t0.append(a)
                t1.append([a[k] + wv.step[k] * (S - 1) for k in range(3)])
                entry.append(ln[3])
    else:
        for r in case.rays:
            t0.append(list(r.start))
            t1.append([r.start[k] + r.step[k] * (S - 1) for k in range(3)])
            entry.append(r.entry)
    t0, t1 = torch.tensor(t0, dtype=F64), torch.tensor(t1, dtype=F64)
    sz = torch.tensor(size, dtype=F64)
    p0, p1 = _coord(t0, sz), _coord(t1, sz)
    seg = p1 - p0
    if case.snap:
        p0 = torch.round(p0 * 2.0 ** 14) / 2.0 ** 14
        seg = torch.round(seg / (S - 1) * 2.0 ** 14) / 2.0 ** 14 * (S - 1)
        assert int((seg != 0).sum(dim=1).max()) <= 1 and S - 1 in (2, 4, 32), "a snapped case marches along one axis with dyadic depths"
    length = seg.norm(dim=1)
    unit = torch.where(length[:, None] > 0, seg / length.clamp(min=1e-30)[:, None], torch.tensor([1.0, 0.0, 0.0], dtype=F64).expand_as(seg))
    n = t0.shape[0]
    enc = 0.5 + 0.5 * torch.rand(n, C, generator=gen)
    rays = Rays(directions=unit.float(), origins=p0.float(), grid_idx=torch.tensor(entry, dtype=torch.long), near=torch.zeros(n),
                far=length.float(), encoding=enc)
    _BUILT[key] = rays
    return rays


def splat_cfg(case: Case):
    return dict(num_samples=case.num_samples, num_samples_inf=0, mask_out_of_bounds_samples=case.mask, contract_coords=False)


def rays_as(rays, dtype):
    r = copy.copy(rays)
    for f in ("directions", "origins", "near", "far", "encoding"):
        setattr(r, f, getattr(r, f).to(dtype))
    return r


# ---- the ledger: geometry ----------------------------------------------------------------------------------------------------------------
def cells_of(rays, num_samples, mask, dtype=torch.float32, unnormalize=O._unnormalize_splatter, sizes_xyz=None):
    """Integer cell (floor of the un-normalised coordinate) of every (ray, sample) along x, y, z for axis sizes ``sizes_xyz`` = (W, H, D),
    and whether the sample is live under the out-of-bounds mask; in ``dtype`` geometry, by the oracle's own functions."""
    r = rays_as(rays, dtype)
    depths = O.ray_depths(r.near, r.far, num_samples, 0, 1e-5)
    points = depths[..., None] * r.directions[:, None] + r.origins[:, None]
    idx = [torch.floor(unnormalize(points[..., k], int(sizes_xyz[k]))).long().numpy() for k in range(3)]
    live = O.in_bounds(points).numpy() if mask else np.ones(points.shape[:-1], dtype=bool)
    return idx, live


@dataclass
class Lanes:
    """[N wave-samples, L lanes]: what every lane of every walk sees.  ``ok``: validity bits of its tap slots (0 for a dead lane);
    ``alive``: the lane holds a ray / a sample at all (a dead lane of a ragged wave repeats ray 0 / the last sample)."""
    b: np.ndarray
    i: Tuple[np.ndarray, np.ndarray, np.ndarray]
    ok: np.ndarray
    alive: np.ndarray
    size: Tuple[int, int, int]     # (W, H, D)


def deal(n_rays, S, dealing, row_length=0):
    """(ray index, sample index, alive) of every lane, [N, L]: "rays32" / "rays16" (csrc/lp_splatter.hip ``splat_fwd_walk_kernel``: wave w
    holds rays w RPW ..), "samples" (``splat_fwd_ray_kernel``: one ray x 32 consecutive samples, the last block clamped to the last
    sample), "bwd" (``splat_bwd_walk_kernel``: 8 rays, ``patch_ray_index`` of csrc/lp_device.h)."""
    if dealing in ("rays32", "rays16", "bwd"):
        L = {"rays32": 32, "rays16": 16, "bwd": 8}[dealing]
        nw = -(-n_rays // L)
        item = np.arange(nw * L).reshape(nw, L)
        alive = item < n_rays
        ray = np.where(alive, patch_ray_index(item, n_rays, row_length) if dealing == "bwd" else item, 0)
        ray = np.repeat(ray[:, None, :], S, axis=1).reshape(nw * S, L)
        alive = np.repeat(alive[:, None, :], S, axis=1).reshape(nw * S, L)
        samp = np.tile(np.repeat(np.arange(S)[:, None], L, axis=1), (nw, 1))
        return ray, samp, alive
    assert dealing == "samples"
    nb = -(-S // 32)
    s = np.arange(nb * 32).reshape(nb, 32)
    alive = np.tile(s < S, (n_rays, 1))
    samp = np.tile(np.minimum(s, S - 1), (n_rays, 1))
    ray = np.repeat(np.arange(n_rays), nb)[:, None] * np.ones((1, 32), dtype=np.int64)
    return ray, samp, alive


def patch_ray_index(idx, n_rays, W):
    """csrc/lp_device.h ``patch_ray_index`` for an array of items"""
    idx = np.asarray(idx, dtype=np.int64)
    if W <= 0:
        return idx
    band_len = 4 * W
    band = idx // band_len
    rem = idx - band * band_len
    x, sub = rem >> 2, rem & 3
    y = np.where(x & 1, 3 - sub, sub)
    return np.where((band + 1) * band_len > n_rays, idx, band * band_len + y * W + x)


def voxel_lanes(rays, case_or_cfg, base, dealing, row_length=0, unnormalize=O._unnormalize_splatter, dtype=torch.float32) -> Lanes:
    B, D, H, W = base
    S, mask = case_or_cfg["num_samples"], case_or_cfg["mask_out_of_bounds_samples"]
    idx, live = cells_of(rays, S, mask, dtype, unnormalize, (W, H, D))
    ray, samp, alive = deal(rays.directions.shape[0], S, dealing, row_length)
    i = tuple(a[ray, samp] for a in idx)
    lv = live[ray, samp] & alive
    okax = []
    for a, n in zip(i, (W, H, D)):
        okax.append(((a >= 0) & (a <= n - 1), (a + 1 >= 0) & (a + 1 <= n - 1)))
    ok = np.zeros(ray.shape, dtype=np.int64)
    for k in range(8):
        ok |= (okax[0][k & 1] & okax[1][(k >> 1) & 1] & okax[2][k >> 2] & lv).astype(np.int64) << k
    return Lanes(rays.grid_idx.numpy().astype(np.int64)[ray], i, ok, alive, (W, H, D))


def plane_lanes(rays, cfg, shape, dealing, row_length=0, unnormalize=O._unnormalize_splatter) -> Lanes:
    """Lanes of a plane grid ``[B, D, H, W]`` with one singleton axis (csrc/lp_device.h ``grid_tapset``: u / v axes); ``i`` = (iu, iv, 0)."""
    B, D, H, W = shape
    S, mask = cfg["num_samples"], cfg["mask_out_of_bounds_samples"]
    idx, live = cells_of(rays, S, mask, torch.float32, unnormalize, (max(W, 1), max(H, 1), max(D, 1)))
    ua, va = (0, 1) if D == 1 else ((0, 2) if H == 1 else (1, 2))
    U, V = (W, H, D)[ua], (W, H, D)[va]
    ray, samp, alive = deal(rays.directions.shape[0], S, dealing, row_length)
    iu, iv = idx[ua][ray, samp], idx[va][ray, samp]
    lv = live[ray, samp] & alive
    oku = ((iu >= 0) & (iu <= U - 1), (iu + 1 >= 0) & (iu + 1 <= U - 1))
    okv = ((iv >= 0) & (iv <= V - 1), (iv + 1 >= 0) & (iv + 1 <= V - 1))
    ok = np.zeros(ray.shape, dtype=np.int64)
    for k in range(4):
        ok |= (oku[k & 1] & okv[k >> 1] & lv).astype(np.int64) << k
    return Lanes(rays.grid_idx.numpy().astype(np.int64)[ray], (iu, iv, np.zeros_like(iu)), ok, alive, (U, V, 1))


# ---- the ledger: predicates ----------------------------------------------------------------------------------------------------------------
def _agree(okp, okn, axis, sign):
    """the carried column's validity agrees between the old and the new cell (lp_splat_walk.h ``up`` / ``down``, ``okAp`` ..)"""
    m0, sh = M0[axis], 1 << axis
    if sign > 0:
        return ((okp & (m0 << sh)) >> sh) == (okn & m0)
    return ((okp & m0) << sh) == (okn & (m0 << sh))


def _carried(okp, okn, axis, sign):
    """the validity bits of the column a +-1 step along ``axis`` keeps in registers (non-zero: something real is carried)"""
    m0, sh = M0[axis], 1 << axis
    return (okn & m0) if sign > 0 else (okn & (m0 << sh))


def _cell_code(i):
    """csrc/lp_device.h ``grid_tapset``: (ix + 1) | (iy + 1) << 10 | (iz + 1) << 20 in 32-bit integers"""
    c = (i[0] + 1).astype(np.int64) | ((i[1] + 1).astype(np.int64) << 10) | ((i[2] + 1).astype(np.int64) << 20)
    return ((c + (1 << 31)) % (1 << 32) - (1 << 31)).astype(np.int64)


def _i32(v):
    return (v + (1 << 31)) % (1 << 32) - (1 << 31)


class Ledger(Counter):
    def reach(self, name, mask):
        n = int(np.count_nonzero(mask))
        if n:
            self[name] += n

    def reached(self):
        return {k for k, v in self.items() if v > 0}


def _rows(L: Lanes):
    W, H, D = L.size
    return L.b * (D * H * W) + (L.i[2] * H + L.i[1]) * W + L.i[0]


def classify_voxel(L: Lanes, walk: str, out: Optional[Ledger] = None) -> Ledger:
    """Counts of the named transitions of one voxel walk over all wave-samples.  ``walk``: "one_axis" (``splat_walk_vox``), "two_axis"
    (``splat_walk_vox_feat2``), "two_axis_diag" (the same with DIAG, the transposed march).  The predicates that do not depend on the
    walk (``run_*``, ``step_*``, ``diag_*``, ``entry_*``, ``alias_*``) are counted for every walk."""
    out = Ledger() if out is None else out
    W, H, D = L.size
    stride = (1, W, H * W)
    row = _rows(L)
    ok, b = L.ok, L.b
    N, n = ok.shape
    okp, okn = ok[:, :-1], ok[:, 1:]
    d = [a[:, 1:] - a[:, :-1] for a in L.i]
    db = b[:, 1:] - b[:, :-1]
    dr = row[:, 1:] - row[:, :-1]
    head = (dr != 0) | (okp != okn)
    both = (okp != 0) & (okn != 0)
    same = db == 0
    absd = [np.abs(x) for x in d]
    moved = absd[0] + absd[1] + absd[2]
    heads = np.concatenate([np.ones((N, 1), dtype=bool), head], axis=1)
    touches = ok != 0
    lane = np.arange(n)[None, :]

    # runs
    out.reach("run_one_run_over_the_whole_wave", ~head.any(axis=1) & touches[:, 0])
    out.reach("run_every_lane_a_head", heads.all(axis=1) & touches.all(axis=1))
    if n >= 16:
        out.reach("run_heads_exactly_at_every_8th_lane", (heads == (lane % 8 == 0)).all(axis=1) & touches.all(axis=1))
    out.reach("run_lane0_dead", ~touches[:, 0] & touches[:, 1:].any(axis=1))
    same_cell = same & (moved == 0)
    out.reach("run_dead_lane_inside_a_run_of_one_cell", same_cell[:, :-1] & same_cell[:, 1:] & touches[:, :-2] & ~touches[:, 1:-1] & touches[:, 2:])
    out.reach("run_all_dead_wave_sample", ~touches.any(axis=1))
    out.reach("run_ragged_last_wave", (~L.alive).any(axis=1) & L.alive.any(axis=1))

    # voxel steps
    for a in range(3):
        others = absd[(a + 1) % 3] + absd[(a + 2) % 3]
        for sg, nm in ((1, "plus"), (-1, "minus")):
            unit = head & same & (d[a] == sg) & (others == 0)
            agree = _agree(okp, okn, a, sg)
            out.reach(f"step_{AXES[a]}_{nm}_equal_validity", unit & agree & both & (_carried(okp, okn, a, sg) != 0))
            refused = unit & ~agree
            lo = np.minimum(L.i[a][:, :-1], L.i[a][:, 1:]) == -1
            hi = np.maximum(L.i[a][:, :-1], L.i[a][:, 1:]) == L.size[a] - 1
            out.reach("step_across_the_low_border_validity_differs", refused & lo)
            out.reach("step_across_the_high_border_validity_differs", refused & hi)
        out.reach(f"step_of_2_along_{AXES[a]}", head & same & (absd[a] == 2) & (others == 0) & both)
    for a, c in ((0, 1), (0, 2), (1, 2)):
        x = 3 - a - c
        for sa in (1, -1):
            for sc in (1, -1):
                dg = head & same & (d[a] == sa) & (d[c] == sc) & (d[x] == 0) & both
                out.reach(f"diag_{AXES[a]}{AXES[c]}_{'p' if sa > 0 else 'm'}{'p' if sc > 0 else 'm'}", dg)
                oa, oc = (sa + 1) >> 1, (sc + 1) >> 1
                so, sn = oa * (1 << a) + oc * (1 << c), (1 - oa) * (1 << a) + (1 - oc) * (1 << c)
                pair = 1 | (1 << (1 << x))
                okD = ((okp >> so) & pair) == ((okn >> sn) & pair)
                out.reach("diag_shared_column_validity_differs", head & same & (d[a] == sa) & (d[c] == sc) & (d[x] == 0) & ~okD)
    out.reach("diag_three_axes", head & same & (absd[0] == 1) & (absd[1] == 1) & (absd[2] == 1) & both)

    # batch entries and row aliases
    other = head & (db != 0)
    out.reach("entry_same_cell_other_entry", other & (moved == 0) & both)
    out.reach("entry_unit_neighbour_in_the_other_entry", other & (moved == 1) & both)
    out.reach("entry_row_delta_equals_one_z_stride", other & (np.abs(dr) == stride[2]) & both)
    alias = head & (dr == 0) & ((okp | okn) != 0)
    out.reach("alias_row_x_end_against_next_y_line", alias & same & (d[1] != 0) & (d[2] == 0))
    out.reach("alias_row_y_end_against_next_z_slab", alias & same & (d[2] != 0))
    out.reach("alias_row_last_corner_against_next_entry", alias & (db != 0))

    packable = W <= PACK_MAX and H <= PACK_MAX and D <= PACK_MAX
    code = _cell_code(L.i)
    dcode = _i32(code[:, 1:] - code[:, :-1])
    for a in range(3):
        if L.size[a] > PACK_MAX:
            out.reach(f"unpackable_axis_{AXES[a]}", np.ones(1, dtype=bool))
            out.reach(f"unpackable_lane_beyond_cell_1023_along_{AXES[a]}", touches & (L.i[a] >= 1023))
            others = absd[(a + 1) % 3] + absd[(a + 2) % 3]
            out.reach(f"unpackable_unit_step_along_{AXES[a]}_not_carried", head & same & (absd[a] == 1) & (others == 0) & both)
        elif L.size[a] == PACK_MAX:
            out.reach(f"packable_edge_1022_along_{AXES[a]}", touches & (L.i[a] == PACK_MAX - 1))
    if not packable:
        out.reach("unpackable_cell_code_delta_looks_like_a_unit_step", head & both & np.isin(np.abs(dcode), (1, 1 << 10, 1 << 20)) & (moved != 1))
        out.reach("unpackable_cell_code_equal_for_different_cells", head & both & (dcode == 0) & (moved != 0))

    if walk == "one_axis":
        _classify_one_axis(out, L, heads, head, both, same, d, absd, dr, dcode, okp, okn, packable, stride)
    else:
        _classify_two_axis(out, L, heads, head, both, same, d, absd, dr, code, okp, okn, packable, stride, walk == "two_axis_diag")
    return out


def _classify_one_axis(out, L, heads, head, both, same, d, absd, dr, dcode, okp, okn, packable, stride):
    """``splat_walk_vox``: A from the first cell change of the wave-sample, then up / down per run head"""
    N, n = heads.shape
    has = head.any(axis=1)
    r1 = np.argmax(head, axis=1)                    # boundary index of the first head behind lane 0
    dc = dcode[np.arange(N), r1]                    # (lane 0's run is one cell: readlane(cell, r1) - readlane(cell, 0))
    A = np.where(np.abs(dc) == (1 << 10), 1, np.where(np.abs(dc) == (1 << 20), 2, 0))
    A = np.where(has, A, 0)
    col = np.arange(n - 1)[None, :]
    later = head & (col > r1[:, None])
    for a in range(3):
        rows = has & (A == a)
        if not rows.any():
            continue
        step = (1 << (10 * a)) if packable else 0x40000000
        up = (dcode == step) & (dr == stride[a]) & _agree(okp, okn, a, 1)
        down = (dcode == -step) & (dr == -stride[a]) & _agree(okp, okn, a, -1)
        sel = rows[:, None]
        real_up = up & (_carried(okp, okn, a, 1) != 0)
        real_down = down & (_carried(okp, okn, a, -1) != 0)
        out.reach(f"one_axis_elects_{AXES[a]}", rows)
        out.reach("one_axis_far_column_carried", head & sel & real_up)
        out.reach("one_axis_near_column_carried", head & sel & real_down)
        out.reach("one_axis_both_columns_flushed", head & sel & ~up & ~down & both)
        out.reach(f"one_axis_elects_{AXES[a]}_then_steps_along_it", later & sel & (real_up | real_down))
        off = same & both & (absd[a] == 0) & ((absd[0] + absd[1] + absd[2]) == 1)
        out.reach(f"one_axis_elects_{AXES[a]}_then_steps_off_it", later & sel & off)
        out.reach("one_axis_unit_step_along_A_in_the_other_entry_refused", head & sel & ~same & both & (np.abs(dcode) == step) & ~up & ~down)
        unit_a = same & (absd[a] == 1) & ((absd[0] + absd[1] + absd[2]) == 1)
        out.reach("one_axis_unit_step_along_A_refused_by_validity", head & sel & unit_a & ~up & ~down & ((okp | okn) != 0))


def _classify_two_axis(out, L, heads, head, both, same, d, absd, dr, code, okp, okn, packable, stride, DIAG):
    """``splat_walk_vox_feat2``: the corner axis X by the counts of head changes per code field, then ``codev`` per run head"""
    N, n = heads.shape
    xr = code[:, 1:] ^ code[:, :-1]
    cnt = [np.count_nonzero(head & (((xr >> (10 * a)) & 0x3FF) != 0), axis=1) for a in range(3)]
    X = np.where((cnt[0] <= cnt[1]) & (cnt[0] <= cnt[2]), 0, np.where(cnt[1] <= cnt[2], 1, 2))
    any_head = head.any(axis=1)
    pre = "two_axis_diag" if DIAG else "two_axis"
    for x in range(3):
        out.reach(f"{pre}_corner_axis_{AXES[x]}", any_head & (X == x))
    out.reach(f"{pre}_three_way_tie", (cnt[0] == cnt[1]) & (cnt[1] == cnt[2]) & (cnt[0] > 0))
    fld = [((code[:, 1:] >> (10 * a)) & 0x3FF) - ((code[:, :-1] >> (10 * a)) & 0x3FF) for a in range(3)]
    for x in range(3):
        rows = any_head & (X == x)
        if not rows.any():
            continue
        sel = rows[:, None]
        A, B = [a for a in range(3) if a != x]
        da, dbb, dx = fld[A], fld[B], fld[x]
        along_a = (dbb == 0) & (dx == 0) & packable
        along_b = (da == 0) & (dx == 0) & packable
        cands = (("A_plus", along_a & (da == 1), stride[A], A, 1), ("A_minus", along_a & (da == -1), -stride[A], A, -1),
                 ("B_plus", along_b & (dbb == 1), stride[B], B, 1), ("B_minus", along_b & (dbb == -1), -stride[B], B, -1))
        taken = np.zeros_like(head)
        for nm, geo, s, ax, sg in cands:
            okc = _agree(okp, okn, ax, sg)
            t = geo & (dr == s) & okc
            taken |= t
            out.reach(f"{pre}_step_{nm}_carried", head & sel & t & (_carried(okp, okn, ax, sg) != 0))
            out.reach(f"{pre}_unit_step_refused_by_validity", head & sel & geo & (dr == s) & ~okc)
            out.reach(f"{pre}_unit_step_refused_by_row_delta", head & sel & geo & (dr != s) & both)
        diag_geo = (dx == 0) & packable & (np.abs(da) == 1) & (np.abs(dbb) == 1) & (dr == da * stride[A] + dbb * stride[B])
        oa, ob = (da + 1) >> 1, (dbb + 1) >> 1
        so, sn = oa * (1 << A) + ob * (1 << B), (1 - oa) * (1 << A) + (1 - ob) * (1 << B)
        pair = 1 | (1 << (1 << x))
        okD = ((okp >> np.clip(so, 0, 7)) & pair) == ((okn >> np.clip(sn, 0, 7)) & pair)
        if DIAG:
            for sa in (1, -1):
                for sb in (1, -1):
                    out.reach(f"{pre}_diagonal_taken_{'p' if sa > 0 else 'm'}{'p' if sb > 0 else 'm'}", head & sel & diag_geo & okD & (da == sa) & (dbb == sb) & both)
            out.reach(f"{pre}_diagonal_refused_shared_column_validity", head & sel & diag_geo & ~okD)
            taken |= diag_geo & okD
        else:
            out.reach(f"{pre}_diagonal_flushes_all", head & sel & diag_geo & both)
        out.reach(f"{pre}_all_columns_flushed", head & sel & ~taken & both)
        true_unit_x = same & (absd[x] == 1) & ((absd[0] + absd[1] + absd[2]) == 1)
        out.reach(f"{pre}_unit_step_along_the_corner_axis", head & sel & true_unit_x & both)
        out.reach(f"{pre}_diagonal_involves_the_corner_axis", head & sel & same & (absd[x] == 1) & ((absd[A] == 1) | (absd[B] == 1)) & both)
    if not packable:
        out.reach(f"{pre}_unpackable_every_carry_off", head & both)


def classify_window(L: Lanes, out: Optional[Ledger] = None) -> Ledger:
    """``splat_walk_vox_weights`` replayed head by head: the 16-cell window of x per (y, z) line pair, its base rule, leaving along x,
    stepping by one y / z line with two pairs kept"""
    out = Ledger() if out is None else out
    W, H, D = L.size
    sv, st = W, H * W
    row = _rows(L)
    iu, iy, iz, b, ok = L.i[0], L.i[1], L.i[2], L.b, L.ok
    N, n = ok.shape
    head = np.concatenate([np.ones((N, 1), dtype=bool), (row[:, 1:] != row[:, :-1]) | (ok[:, 1:] != ok[:, :-1])], axis=1)
    touches = ok != 0
    out.reach("window_lane_at_iu_minus_1", touches & (iu == -1))
    out.reach("window_lane_at_iu_last", touches & (iu == W - 1))

    def base_of(u, tag):
        if (u & 15) == 15:
            out[f"window_base_rule_iu_and_15_is_15{tag}"] += 1
            if u == -1:
                out["window_base_at_minus_1"] += 1
            return u
        out["window_base_aligned"] += 1
        return u & ~15

    for w in range(N):
        hs = np.nonzero(head[w])[0]
        s_iu, s_row = int(iu[w, 0]), int(row[w, 0])
        wb = base_of(s_iu, "")
        rowb = s_row - s_iu
        line = (int(b[w, 0]), int(iy[w, 0]), int(iz[w, 0]))
        last_iu = s_iu
        for rr in hs[1:]:
            n_iu, n_row = int(iu[w, rr]), int(row[w, rr])
            n_line = (int(b[w, rr]), int(iy[w, rr]), int(iz[w, rr]))
            live_pair = bool(ok[w, rr] != 0 and ok[w, rr - 1] != 0)
            dl = (n_row - n_iu) - rowb
            out_x = not (0 <= n_iu - wb < 15)
            line_step = dl in (sv, -sv, st, -st)
            if live_pair and dl == 0:
                if last_iu == 14 and n_iu == 15:
                    out["window_iu_14_to_15"] += 1
                if last_iu == 15 and n_iu == 16:
                    out["window_iu_15_to_16"] += 1
            if dl == 0 and not out_x:
                out["window_head_stays_inside"] += live_pair
            elif line_step and not out_x:
                true = (n_line[0] == line[0]) and ((n_line[1] - line[1], n_line[2] - line[2]) in ((1, 0), (-1, 0), (0, 1), (0, -1))) \
                    and dl == (n_line[1] - line[1]) * sv + (n_line[2] - line[2]) * st
                if true:
                    nm = {sv: "y_plus", -sv: "y_minus", st: "z_plus", -st: "z_minus"}[dl]
                    out[f"window_line_step_{nm}"] += live_pair
                else:
                    out["window_line_step_only_by_a_row_alias"] += 1
                    if n_line[0] != line[0]:
                        out["window_line_step_because_the_entry_changed"] += 1
                rowb += dl
            else:
                if dl == 0:
                    out["window_left_along_x_forward" if n_iu - wb >= 15 else "window_left_along_x_backward"] += live_pair
                    if abs(n_iu - last_iu) >= 15:
                        out["window_left_along_x_by_15_or_more"] += live_pair
                elif line_step:
                    out["window_line_step_together_with_leaving_x"] += live_pair
                else:
                    out["window_left_for_another_line"] += live_pair
                wb = base_of(n_iu, "_on_rebase")
                rowb = n_row - n_iu
            line = n_line
            last_iu = n_iu
    return out


def classify_plane(L: Lanes, out: Optional[Ledger] = None) -> Ledger:
    """``splat_walk`` (``splat_walk_slots``) on a plane grid: runs of one row and their heads"""
    out = Ledger() if out is None else out
    U, V, _ = L.size
    row = plane_rows(L)
    ok = L.ok
    okp, okn = ok[:, :-1], ok[:, 1:]
    dr = row[:, 1:] - row[:, :-1]
    head = (dr != 0) | (okp != okn)
    both = (okp != 0) & (okn != 0)
    db = L.b[:, 1:] - L.b[:, :-1]
    t = ok != 0
    out.reach("plane_same_row_merged", ~head & both)
    out.reach("plane_row_change", head & (db == 0) & both & (dr != 0))
    out.reach("plane_border_u_low", t & (L.i[0] == -1))
    out.reach("plane_border_u_high", t & (L.i[0] == U - 1))
    out.reach("plane_border_v_low", t & (L.i[1] == -1))
    out.reach("plane_border_v_high", t & (L.i[1] == V - 1))
    out.reach("plane_other_entry", head & (db != 0) & both)
    out.reach("plane_dead_lane_next_to_a_live_one", (okp != 0) != (okn != 0))
    out.reach("plane_row_alias_u_end_against_next_v_line", head & (dr == 0) & (db == 0) & ((okp | okn) != 0))
    return out


def plane_rows(L: Lanes):
    """row of the first tap of every lane of ``plane_lanes``"""
    U, V, _ = L.size
    return L.b * (U * V) + L.i[1] * U + L.i[0]


def triplane_sentinel_rows(rays, cfg, base, dealing):
    """csrc/lp_mfma_common.h ``scatter_triplane`` (the tuned Renderer's backward on a canonical triplane, Renderer convention): per plane
    xy, xz, yz the row of every lane, [N, L] -- the first cell of each axis clamped to [0, size - 2] (``axis_norm``: a border cell is
    re-expressed with all four corners in range), the sentinel -1 where the lane is not live or an axis has no tap in range."""
    B, D, H, W = base
    S, mask = cfg["num_samples"], cfg["mask_out_of_bounds_samples"]
    idx, live = cells_of(rays, S, mask, torch.float32, O._unnormalize_renderer, (W, H, D))
    ray, samp, alive = deal(rays.directions.shape[0], S, dealing)
    lv = live[ray, samp] & alive
    b = rays.grid_idx.numpy().astype(np.int64)[ray]
    cell, dead = [], []
    for a, n in zip(idx, (W, H, D)):
        i0 = a[ray, samp]
        dead.append(~(((i0 >= 0) & (i0 <= n - 1)) | ((i0 + 1 >= 0) & (i0 + 1 <= n - 1))))
        cell.append(np.clip(i0, 0, n - 2))
    (ax, ay, az), (dx, dy, dz) = cell, dead
    return [np.where(~lv | dx | dy, -1, (b * H + ay) * W + ax), np.where(~lv | dx | dz, -1, (b * D + az) * W + ax),
            np.where(~lv | dy | dz, -1, (b * D + az) * H + ay)]


def classify_slot_runs(row, ok, out: Optional[Ledger] = None) -> Ledger:
    """The branches of a per-slot run loop (csrc/lp_splat_walk.h ``splat_walk_slots``, its written-out forms in csrc/lp_mfma_common.h) over the wave-samples ``[N, L]`` of one grid: a head is lane 0 and
    every lane whose row or validity bits differ from its predecessor's (``run_head``); a run is live if its validity bits are not 0.
    For the sentinel-row policy pass ``ok = row >= 0``."""
    out = Ledger() if out is None else out
    ok = np.asarray(ok).astype(np.int64)
    head = np.concatenate([np.ones((row.shape[0], 1), dtype=bool), (row[:, 1:] != row[:, :-1]) | (ok[:, 1:] != ok[:, :-1])], axis=1)
    for w in range(row.shape[0]):
        live = ok[w, np.flatnonzero(head[w])] != 0
        out["slot_single_live_run"] += int(len(live) == 1 and live[0])
        out["slot_single_dead_run"] += int(len(live) == 1 and not live[0])
        out["slot_several_runs"] += int(len(live) >= 2)
        out["slot_dead_run_between_two_live_runs"] += int(np.count_nonzero(live[:-2] & ~live[1:-1] & live[2:]))
    return out


def backward_segments(n_rays, S):
    """csrc/lp_splatter.hip ``splat_segments`` for a batch below one round of resident waves"""
    ray_blocks = -(-n_rays // 32)
    n = 768 // max(1, (ray_blocks + 1) // 2)
    return max(1, min(n, S // 16))


def classify_backward(L: Lanes, n_rays, S, row_length, out: Optional[Ledger] = None) -> Ledger:
    """``splat_bwd_walk_kernel``: 8 rays per wave, blocks of 8 samples; a run reads its rows once, a head reads again"""
    out = Ledger() if out is None else out
    row = _rows(L)
    ok = L.ok
    okp, okn = ok[:, :-1], ok[:, 1:]
    head = (row[:, 1:] != row[:, :-1]) | (okp != okn)
    both = (okp != 0) & (okn != 0)
    t = ok != 0
    out.reach("backward_run_of_several_rays_reads_once", ~head & both)
    out.reach("backward_head_reads_again", head & both)
    out.reach("backward_head_in_the_other_entry", head & both & (L.b[:, 1:] != L.b[:, :-1]))
    out.reach("backward_dead_sample_of_the_wave_skipped", ~t.any(axis=1))
    out.reach("backward_lane0_dead", ~t[:, 0] & t[:, 1:].any(axis=1))
    out.reach("backward_ragged_last_wave", (~L.alive).any(axis=1) & L.alive.any(axis=1))
    if S % 8:
        out["backward_last_sample_block_partial"] += 1
    if backward_segments(n_rays, S) > 1:
        out["backward_several_segments"] += 1
    else:
        out["backward_one_segment"] += 1
    if row_length > 0:
        items = np.arange(n_rays)
        moved = patch_ray_index(items, n_rays, row_length) != items
        out.reach("backward_patch_order_2x4_pixels", moved)
        if n_rays % (4 * row_length):
            out.reach("backward_patch_tail_keeps_scanline_order", ~moved[-(n_rays % (4 * row_length)):])
        else:
            out["backward_patch_image_height_multiple_of_4"] += 1
    return out


# ---- which walk a launch takes (csrc/lp_splatter.hip ``splatter_forward_launch``) ----------------------------------------------------------
def forward_walks(C, form, order):
    """(dealing, voxel walk) of the plain Splatter's forward for a channel count, a grid-list form and a march order"""
    dealing = "samples" if order == "samples" else ("rays16" if C == 64 else "rays32")
    if form == "voxel" and C in (32, 64):
        return dealing, ("two_axis_diag" if order == "samples" else "two_axis")
    return dealing, "one_axis"


def ledger_of(case: Case, C: int, form: str = "voxel", order: Optional[str] = None, rays=None) -> Ledger:
    """Every predicate the plain Splatter's forward reaches on ``case`` with this channel count and grid-list form"""
    order = order or case.order
    rays = build_rays(case, C) if rays is None else rays
    cfg = splat_cfg(case)
    dealing, walk = forward_walks(C, form, order)
    out = Ledger()
    for gs in grid_sizes(case, C, form):
        B, D, H, W, _ = gs
        if D > 1 and H > 1 and W > 1:
            L = voxel_lanes(rays, cfg, (B, D, H, W), dealing)
            classify_voxel(L, walk, out)
            classify_window(L, out)
        else:
            classify_plane(plane_lanes(rays, cfg, (B, D, H, W), dealing), out)
    n = rays.directions.shape[0]
    if order == "rays" and n % 128 and n % 32 and n % 16:
        out["run_ray_count_no_multiple_of_the_block_or_the_wave"] += 1
    if order == "samples" and case.num_samples % 32:
        out.reach("transposed_last_block_has_dead_lanes", np.ones(1, dtype=bool))
    return out


def backward_ledger_of(case: Case, C: int, row_length: int = 0) -> Ledger:
    rays = build_rays(case, C)
    L = voxel_lanes(rays, splat_cfg(case), case.base, "bwd", row_length)
    return classify_backward(L, rays.directions.shape[0], case.num_samples, row_length)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
G0 = (2, 6, 7, 20)
DEAD_LO, DEAD_HI, IN_LO, IN_HI = 0.3, 0.7, 0.6, 0.4   # fractional parts in the cells -1 / size - 1: out of bounds, inside


def _pad(lanes, cell=(12, 2, 1), b=0):
    lanes = tuple(lanes)
    assert len(lanes) <= 32, len(lanes)
    return lanes + rep(cell, 32 - len(lanes), b)


def _main_waves():
    X, Y, Z = (1, 0, 0), (0, 1, 0), (0, 0, 1)
    neg = lambda v: tuple(-c for c in v)  # noqa: E731
    w = []
    w.append(Wave(rep((5, 3, 1), 32)))                                                       # one run over the whole wave
    w.append(Wave(tuple((2 * (r % 8) + 1, 1 + r // 8, 2, 0) for r in range(32))))            # every lane a head, steps of 2
    # axis election: 4 lanes per cell, (c0, +a, +a, +off) twice per wave -- the same in a 16-ray and a 32-ray wave
    w.append(Wave(path((4, 3, 2), [X, X, Y], 4) + path((9, 2, 2), [neg(X), neg(X), neg(Y)], 4)))
    w.append(Wave(path((4, 1, 2), [Y, Y, Z], 4) + path((4, 5, 3), [neg(Y), neg(Y), neg(Z)], 4)))
    w.append(Wave(path((9, 3, 0), [Z, Z, X], 4) + path((11, 3, 4), [neg(Z), neg(Z), neg(X)], 4)))
    w.append(Wave(path((3, 2, 1), [X, Y, Z], 4) + path((8, 4, 3), [X, Y, Z], 4)))              # three-way tie
    w.append(Wave(path((3, 2, 1), [X, Y, Z], 8)))                                             # heads exactly at 8 / 16 / 24
    # (two lanes per cell; the step in the middle sits on the boundary of two 16-ray waves: the jump of 2, which other waves have too)
    diag = [(1, 1, 0), (1, -1, 0), (-1, 1, 0), (-1, -1, 0), (1, 0, 1), (1, 0, -1), (-1, 0, 1), (2, 0, 0), (-1, 0, -1), (0, 1, 1), (0, 1, -1),
            (0, -1, 1), (0, -1, -1), (1, 1, 1), (-1, -1, -1)]
    w.append(Wave(path((8, 3, 2), diag, 2)))
    w.append(Wave(path((8, 3, 2), [(0, 2, 0), (0, 0, 2), (0, -2, 0), (0, 0, -2), (-2, 0, 0), (1, 1, 1), (1, -1, 1)], 4)))
    # borders: points out of bounds under the mask (dead lanes), partly valid cells without it
    lo_dead, hi_dead, lo_in, hi_in = (DEAD_LO, None, None), (DEAD_HI, None, None), (IN_LO, None, None), (IN_HI, None, None)
    bl = rep((-1, 3, 2), 1, frac=lo_dead) + rep((0, 3, 2), 3) + rep((-1, 3, 2), 1, frac=lo_dead) + rep((-1, 3, 2), 2, frac=lo_in) + rep((0, 3, 2), 2)
    bl += rep((18, 3, 2), 2) + rep((19, 3, 2), 2, frac=hi_in) + rep((19, 3, 2), 1, frac=hi_dead) + rep((19, 3, 2), 2, frac=hi_in)
    bl += rep((18, 3, 2), 2) + rep((19, 3, 2), 1, frac=hi_dead)
    bl += rep((6, 0, 2), 2) + rep((6, -1, 2), 1, frac=(None, DEAD_LO, None)) + rep((6, 5, 2), 2) + rep((6, 6, 2), 1, frac=(None, DEAD_HI, None))
    bl += rep((7, 3, 0), 2) + rep((7, 3, -1), 1, frac=(None, None, DEAD_LO)) + rep((7, 3, 4), 2) + rep((7, 3, 5), 1, frac=(None, None, DEAD_HI))
    w.append(Wave(_pad(bl)))
    # a diagonal whose shared column differs in validity: into a dead corner cell
    w.append(Wave(_pad(rep((18, 5, 2), 3) + rep((19, 6, 2), 2, frac=(DEAD_HI, DEAD_HI, None)) + rep((18, 5, 2), 2)
                       + rep((0, 0, 2), 2) + rep((-1, -1, 2), 2, frac=(DEAD_LO, DEAD_LO, None)) + rep((0, 0, 2), 2)
                       + rep((3, 5, 4), 2) + rep((3, 6, 5), 2, frac=(None, DEAD_HI, DEAD_HI)) + rep((3, 5, 4), 2))))
    # batch entries and row aliases
    en = rep((5, 3, 2), 3, 0) + rep((5, 3, 2), 3, 1) + rep((6, 3, 2), 2, 0) + rep((6, 3, 2), 2, 1) + rep((6, 4, 2), 2, 0)
    en += rep((7, 2, 5), 2, 0) + rep((7, 2, 0), 2, 1)                                                     # last z slab, first of the next entry
    en += rep((19, 2, 3), 2, 0) + rep((-1, 3, 3), 2, 0)                                                   # (iy, W - 1) against (iy + 1, -1)
    en += rep((4, 6, 2), 2, 0) + rep((4, -1, 3), 2, 0)                                                    # (iz, H - 1) against (iz + 1, -1)
    en += rep((19, 6, 5), 2, 0) + rep((-1, 0, 0), 2, 1)                                                   # last corner against the next entry
    w.append(Wave(_pad(en, b=1)))
    w.append(Wave(_pad(en, b=1)))
    # the weight window on W = 20: a sweep over every iu, then back over a y line
    w.append(Wave(_pad(tuple((ix, 2, 3, 0) for ix in range(-1, 20)) + tuple((ix, 3, 3, 0) for ix in (19, 4, 3, 2, 1, 0, -1)))))
    w.append(Wave(rep((25, 3, 2), 32)))                                                       # a wave that never touches the grid
    w.append(Wave(path((10, 4, 3), [X, Y], 4) + rep((11, 5, 3), 1)))                           # the ragged last wave: 13 rays
    # (the step per sample is dealt here:) every wave moves along all three axes from sample to sample: a plane grid then sees a new cell per sample too (a step along one axis
    # stacks all S samples of a wave on one cell of the plane across it, and the largest entry buries the smallest contribution)
    cyc = [(1, 1, 1), (1, -1, 1), (-1, 1, 1), (1, 1, -1), (-1, -1, 1), (1, -1, -1), (-1, 1, -1)]
    return tuple(Wave(x.lanes, cyc[i % len(cyc)]) for i, x in enumerate(w))


def _window_waves(W, D=3, H=4):
    """the weight window on a grid of W cells along x: every iu from -1 to W - 1 up and down, line steps with and without leaving x,
    a line step that is one only because the entry changed"""
    w = []
    per = W + 1
    up = tuple((-1 + r % per, (r // per) % 3, min(r // (3 * per), D - 1), 0) for r in range(64))
    w.append(Wave(up[:32], (0, 0, 1)))
    w.append(Wave(up[32:], (0, 0, 1)))
    w.append(Wave(tuple((W - 1 - r % per, 1 + (r // per) % 2, 1, 0) for r in range(32)), (0, 0, -1)))
    x0, far = min(5, W - 1), min(W - 1, 16)
    ln = rep((x0, 1, 1), 2) + rep((x0, 2, 1), 2) + rep((x0, 1, 1), 2) + rep((x0, 1, 2), 2) + rep((x0, 1, 1), 2)   # +y -y +z -z
    ln += rep((-1, 1, 1), 2) + rep((far, 2, 1), 2)              # a line step together with leaving x (W >= 15)
    ln += rep((-1, 2, 1), 2) + rep((far, 2, 1), 2)              # leaving x by 15 or more on one line
    ln += rep((x0, 1, D - 1), 2, 0) + rep((x0, 1, 0), 2, 1)     # dl == one z stride only because the entry changed
    ln += rep((x0, 2, 0), 2, 1) + rep((x0, 2, D - 1), 2, 0)
    w.append(Wave(_pad(ln, cell=(0, 0, 0)), (0, 0, 0)))
    w.append(Wave(_pad(ln, cell=(0, 0, 0))[:21], (0, 1, 0)))
    return tuple(w)


def _unpackable_waves(axis, n):
    """lanes around cell 1023 and at the far end of an axis of n cells (n = 1022: the largest packable size), unit steps along it and
    off it, a jump of exactly 1024 cells (the cell code's delta of a z step of 1024 is the walk's unpackable step constant)"""
    def cell(p, o1=0, o2=1):
        c = [o1, o2]
        c.insert(axis, p)
        return tuple(c)
    short = (1, 0, 0)[axis]                       # the 2-cell axis (``o1``): the march goes along it, one cell per sample
    fwd = tuple(int(k == short) for k in range(3))
    pos = [1019, 1020, 1021] + ([1022, 1023, 1024, 1025] if n > 1025 else []) + [n - 3, n - 2, n - 1]
    pos = [p for p in pos if p < n]
    a = ()
    for p in pos:
        a += rep(cell(p), 2)
    a += rep(cell(pos[-1], 1), 2) + rep(cell(pos[-1], 1, 2), 2) + rep(cell(pos[-1] - 1, 1, 2), 2)
    wv = [Wave(_pad(a[:32], cell=cell(3)), fwd)]
    b = rep(cell(100), 4) + rep(cell(100 + 1024), 4) if n > 1200 else rep(cell(100), 4) + rep(cell(101), 4)
    b += rep(cell(n - 2, 0), 3) + rep(cell(n - 1, 0), 3) + rep(cell(n - 1, 0), 3, 1) + rep(cell(-1, 0), 2) + rep(cell(0, 0), 3)
    wv.append(Wave(b[:32], fwd))
    return tuple(wv)


def _unpackable_base(axis, n):
    dims = {0: (3, 2, n), 1: (3, n, 2), 2: (n, 3, 2)}[axis]   # (D, H, W): one axis of n cells, one of 2, one of 3
    return (2,) + dims


def _patch_image(hgt, wid=8):
    """an image of hgt x wid pixels whose 2 x 2 pixel blocks share a cell (the backward's 2 x 4 pixel patches merge them)"""
    return tuple((3 + px // 2, 1 + py // 2, 2, 0) for py in range(hgt) for px in range(wid))


def _transposed_rays(W=20):
    r = []
    h = 0.5
    for a in range(3):
        for sg in (1, -1):
            # dwell: a quarter of a cell per sample; unit steps from outside the grid through it and out again; a jump of 2
            st = [0.0, 0.0, 0.0]
            st[a] = 0.25 * sg
            s0 = [5 + h, 3 + h, 2 + h]
            s0[a] = (1.125 if sg > 0 else (4.875 if a else 9.875))
            r.append(RayScript(tuple(s0), tuple(st), a & 1))
            st[a] = 1.0 * sg
            s0[a] = (-3 + 0.4) if sg > 0 else ((W, 7, 6)[a] + 2 + 0.4)
            r.append(RayScript(tuple(s0), tuple(st), 0))
        st = [0.0, 0.0, 0.0]
        st[a] = 2.0
        s0 = [5 + h, 3 + h, 2 + h]
        s0[a] = -2 + 0.35
        r.append(RayScript(tuple(s0), tuple(st), 1))
    for a, c in ((0, 1), (0, 2), (1, 2)):
        for sa in (1, -1):
            for sc in (1, -1):
                st, s0 = [0.0, 0.0, 0.0], [6 + 0.4, 3 + 0.6, 2 + 0.45]
                st[a], st[c] = float(sa), float(sc)
                s0[a] = (-2 + 0.4) if sa > 0 else ((W, 7, 6)[a] + 0.6)
                s0[c] = (-2 + 0.55) if sc > 0 else ((W, 7, 6)[c] + 0.45)
                r.append(RayScript(tuple(s0), tuple(st), 0))
    r.append(RayScript((-2 + 0.4, -2 + 0.5, -2 + 0.6), (1.0, 1.0, 1.0), 0))                    # the three-axis diagonal
    r.append(RayScript((8 + 0.4, 7 + 0.5, 6 + 0.6), (-1.0, -1.0, -1.0), 1))
    r.append(RayScript((-1 + 0.6, -1 + 0.55, 0.125), (1.0, 1.0, 0.25), 0))                     # every fourth step involves the third axis
    r.append(RayScript((2 + 0.4, 0.125, 5 + 0.4), (1.0, 0.25, -1.0), 1))
    r.append(RayScript((0.125, 6 + 0.4, 0 + 0.6), (0.25, -1.0, 1.0), 0))
    r.append(RayScript((5.3, 3.5, 2.5), (0.01, 0.0, 0.0), 1))                                  # one cell for the whole march
    r.append(RayScript((4.0625, 4.5, 3.5), (0.125, 0.0, 0.0), 1))                              # heads exactly at lanes 8 / 16 / 24
    r.append(RayScript((-3 + 0.6, 1.5, 4.5), (1.0, 0.0, 0.0), 1))                              # leaves the bounds in the last cell
    # two and three rates: unit steps off the elected axis, and along the corner axis of the two-axis walk
    r.append(RayScript((1.25, 1.375, 0.5), (0.5, 0.25, 0.0), 1))
    r.append(RayScript((12.5, 0.25, 0.375), (0.0, 0.5, 0.25), 1))
    r.append(RayScript((13.375, 5.5, 0.25), (0.25, 0.0, 0.5), 1))
    r.append(RayScript((10.25, 0.375, 0.875), (0.5, 0.25, 0.25), 1))
    return tuple(r)


CASES: Dict[str, Case] = {}


def _add(c: Case):
    assert c.name not in CASES
    CASES[c.name] = c


_add(Case("main", G0, 8, False, waves=_main_waves()))
_add(Case("main_mask", G0, 8, True, waves=_main_waves(), seed=1))
for _W in (2, 15, 16, 17, 33):
    _add(Case(f"window_w{_W}", (2, 3, 4, _W), 4, False, waves=_window_waves(_W), seed=10 + _W))
for _ax in range(3):
    for _n in (1022, 1023, 1500):
        _add(Case(f"long_{AXES[_ax]}{_n}", _unpackable_base(_ax, _n), 3, False, waves=_unpackable_waves(_ax, _n), seed=100 + _n + _ax, snap=True))
_add(Case("transposed_s33", G0, 33, False, rays=_transposed_rays()))
_add(Case("transposed_s40_mask", G0, 40, True, rays=_transposed_rays(), seed=3))
_add(Case("transposed_w33_s40", (2, 6, 7, 33), 40, False, rays=_transposed_rays(33), seed=4))
for _ax in range(3):   # rays along the long axis: across cell 1023, out at the far end, and one that dwells
    def _at(p, _ax=_ax):
        c = [0.5, 1.5]
        c.insert(_ax, p)
        return tuple(c)
    _st = tuple(float(k == _ax) for k in range(3))
    _add(Case(f"transposed_long_{AXES[_ax]}1500", _unpackable_base(_ax, 1500), 33, False, seed=5 + _ax, snap=True,
              rays=(RayScript(_at(1500 - 25 + 0.35), _st, 0), RayScript(_at(1008 + 0.35), _st, 1),
                    RayScript(_at(1019 + 0.25), tuple(0.5 * v for v in _st), 0))))
_add(Case("patch_8x8", G0, 8, False, waves=(Wave(_patch_image(8)[:32], (0, 0, 1)), Wave(_patch_image(8)[32:], (0, 0, 1))), row_length=8, seed=7))
_add(Case("patch_6x8", G0, 8, False, waves=(Wave(_patch_image(6)[:32], (0, 0, 1)), Wave(_patch_image(6)[32:], (0, 0, 1))), row_length=8, seed=8))

RAY_ORDER_CASES = [n for n, c in CASES.items() if c.order == "rays" and not c.row_length]
TRANSPOSED_CASES = [n for n, c in CASES.items() if c.order == "samples"]
LONG_CASES = [n for n in CASES if n.startswith("long_")]
WINDOW_CASES = [n for n in CASES if n.startswith("window_")]

# ---- the forward launches of the plain Splatter: (case, C, grid-list form) -------------------------------------------------------------------
FORWARD_RAYS = [(n, C, "voxel") for n in RAY_ORDER_CASES for C in (16, 32, 64)] + \
    [(n, C, "voxel+xy") for n in ("main", "main_mask", "window_w17") for C in (32, 64)] + [(n, 16, "triplane") for n in ("main", "main_mask")]
FORWARD_SAMPLES = [(n, C, "voxel") for n in TRANSPOSED_CASES for C in (16, 32, 64)] + [("transposed_s40_mask", 32, "voxel+xy")]
# backward: (case, C, row length)
BACKWARD = [(n, C, 0) for n in ("main", "main_mask", "transposed_s33", "transposed_s40_mask") for C in (16, 32, 64)] + \
    [(n, C, 8) for n in ("patch_8x8", "patch_6x8") for C in (16, 32, 64)]


# ---- what every walk has to be driven through: the union over the table reaches all of it (tests/test_walk_transitions_host.py) ---------------
_STEPS = [f"step_{a}_{s}_equal_validity" for a in AXES for s in ("plus", "minus")] + \
    ["step_across_the_low_border_validity_differs", "step_across_the_high_border_validity_differs"] + [f"step_of_2_along_{a}" for a in AXES] + \
    [f"diag_{p}_{s}" for p in ("xy", "xz", "yz") for s in ("pp", "pm", "mp", "mm")] + ["diag_three_axes", "diag_shared_column_validity_differs"]
_RUNS = ["run_one_run_over_the_whole_wave", "run_every_lane_a_head", "run_heads_exactly_at_every_8th_lane", "run_lane0_dead",
         "run_all_dead_wave_sample", "run_ragged_last_wave"]
_RUNS_RAYS = _RUNS + ["run_dead_lane_inside_a_run_of_one_cell", "run_ray_count_no_multiple_of_the_block_or_the_wave"]
_ENTRIES = ["entry_same_cell_other_entry", "entry_unit_neighbour_in_the_other_entry", "entry_row_delta_equals_one_z_stride",
            "alias_row_x_end_against_next_y_line", "alias_row_y_end_against_next_z_slab", "alias_row_last_corner_against_next_entry"]
_ONE = [f"one_axis_elects_{a}{t}" for a in AXES for t in ("", "_then_steps_along_it", "_then_steps_off_it")] + \
    ["one_axis_far_column_carried", "one_axis_near_column_carried", "one_axis_both_columns_flushed", "one_axis_unit_step_along_A_refused_by_validity"]
_TWO = [f"_corner_axis_{a}" for a in AXES] + ["_three_way_tie", "_step_A_plus_carried", "_step_A_minus_carried", "_step_B_plus_carried",
                                              "_step_B_minus_carried", "_unit_step_refused_by_validity", "_all_columns_flushed",
                                              "_unit_step_along_the_corner_axis", "_diagonal_involves_the_corner_axis"]
_WINDOW = ["window_lane_at_iu_minus_1", "window_lane_at_iu_last", "window_base_at_minus_1", "window_base_rule_iu_and_15_is_15",
           "window_base_rule_iu_and_15_is_15_on_rebase", "window_base_aligned", "window_iu_14_to_15", "window_iu_15_to_16",
           "window_head_stays_inside", "window_left_along_x_forward", "window_left_along_x_backward", "window_left_for_another_line",
           "window_line_step_together_with_leaving_x"] + [f"window_line_step_{a}_{s}" for a in "yz" for s in ("plus", "minus")]
_LONG = [f"{p}{a}" for a in AXES for p in ("unpackable_axis_", "unpackable_lane_beyond_cell_1023_along_", "packable_edge_1022_along_")] + \
    [f"unpackable_unit_step_along_{a}_not_carried" for a in AXES]
_PLANE = ["plane_same_row_merged", "plane_row_change", "plane_border_u_low", "plane_border_u_high", "plane_border_v_low",
          "plane_border_v_high", "plane_dead_lane_next_to_a_live_one"]
REQUIRED: Dict[str, List[str]] = {
    # march_order="rays"
    "one_axis": _RUNS_RAYS + _STEPS + _ENTRIES + _ONE + ["one_axis_unit_step_along_A_in_the_other_entry_refused"] + _LONG,
    "two_axis": _RUNS_RAYS + _STEPS + _ENTRIES + ["two_axis" + t for t in _TWO] + ["two_axis_unit_step_refused_by_row_delta",
                                                                                    "two_axis_diagonal_flushes_all", "two_axis_unpackable_every_carry_off"] + _LONG,
    "window": _WINDOW + ["window_left_along_x_by_15_or_more", "window_line_step_only_by_a_row_alias", "window_line_step_because_the_entry_changed"],
    "plane": _PLANE + ["plane_other_entry", "plane_row_alias_u_end_against_next_v_line"],
    # march_order="samples"
    "one_axis_transposed": _RUNS + _STEPS + _ONE + ["transposed_last_block_has_dead_lanes"] + [n for n in _LONG if not n.startswith("packable")],
    "two_axis_diag": _RUNS + _STEPS + ["two_axis_diag" + t for t in _TWO] + [f"two_axis_diag_diagonal_taken_{s}" for s in ("pp", "pm", "mp", "mm")] +
    ["two_axis_diag_diagonal_refused_shared_column_validity", "two_axis_diag_unpackable_every_carry_off", "transposed_last_block_has_dead_lanes"] +
    [n for n in _LONG if not n.startswith("packable")],
    "window_transposed": _WINDOW,
    "plane_transposed": _PLANE,
    "backward": ["backward_run_of_several_rays_reads_once", "backward_head_reads_again", "backward_head_in_the_other_entry",
                 "backward_dead_sample_of_the_wave_skipped", "backward_lane0_dead", "backward_ragged_last_wave", "backward_last_sample_block_partial",
                 "backward_several_segments", "backward_one_segment", "backward_patch_order_2x4_pixels", "backward_patch_tail_keeps_scanline_order",
                 "backward_patch_image_height_multiple_of_4"],
}
GRID_WIDTHS_REQUIRED = (2, 15, 16, 17, 33)       # along x, for the weight window
LONG_AXES_REQUIRED = (1022, 1023, 1500)          # each of x, y, z in turn


def walk_keys(C, form, order):
    """the REQUIRED tables a forward launch counts towards"""
    _, walk = forward_walks(C, form, order)
    t = order == "samples"
    keys = [("one_axis_transposed" if t else "one_axis") if walk == "one_axis" else walk]
    if form in ("voxel", "voxel+xy"):
        keys.append("window_transposed" if t else "window")
    if form in ("voxel+xy", "triplane"):
        keys.append("plane_transposed" if t else "plane")
    return keys

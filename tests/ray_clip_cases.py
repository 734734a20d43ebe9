"""Seeded cases, the fp64 oracle and the checks of the ray clip (lp_rays_clip / lp.clip_rays_to_scaffold); no GPU here.

Oracle (brute force over cells: it needs no walk of its own to be trusted).  For each ray and each occupied cell (value != 0) of its
scene, the slab interval of the cell's box in fp64 -- a component d_a == 0 is inside iff o_a lies in the slab -- intersected with
[near, far].  O is the union of these intersections: hit64 = |O| > 0, near* = min O, far* = max O.  A ray with a NaN / Inf entry, with
far < near or with grid_idx outside [0, B) has an empty O.

Scaffolds (the smallest shapes with unequal axes, a batch stride and the degenerate walks): SCAFFOLDS below; "box" is no scaffold, which
the oracle treats as one occupied cell [-1, 1]^3.

Rays per case: R = 257 (no multiple of 64 or 256), the mix of `_rays` below: origins outside the box, inside it and inside an occupied
cell; rays that miss the box; negative directions; |d| in {0.3, 1, 3}; one, two and three zero direction components (the origin
coordinates of those axes at least 1e-3 h -- in fact 0.05 of a cell -- from every cell face); near inside the box; far before the box;
far inside the object; far < near; 8 ill-conditioned rays (one component 0 < |d_a| < 1e-3 |d|_inf); 4 rays with NaN or Inf entries;
2 rays with grid_idx out of range.  The far < near rays are misses by definition, and the conservativeness test looks at the samples
the Renderer's formula near + lin01 * (far - near) places for them too: they keep both ends in front of the box, so that this degenerate
schedule samples nothing.  Every case runs at pad in PADS.

Ambiguous rays (left out of the `hit` and tightness comparisons only, never of the conservativeness check): O is not empty and
|O| < 1e-4 h / |d|, or near or far lies within 1e-5 (far - near) of an end of an occupied cell's interval.  (An empty O is a plain miss,
not an ambiguity.)  At most 2 % of a case's rays may be ambiguous: a condition on the inputs, checked from the oracle alone by
tests/test_ray_clip_host.py::test_cases_are_unambiguous; a seed that fails it is changed, never the cap.

Tightness tolerance (derived, not tuned): tol = 16 * 2^-24 * max_a (1 + |o_a|) / |d_a| over the non-zero components + 4 * 2^-24 * |t|:
the rounding of one directly computed crossing (plane - o_a) / d_a -- the plane, the difference (at most 1 + |o_a|) and the quotient
each round once -- with a margin of a few ulp.  expected - 2 tol <= near' <= expected + tol with expected = max(near, near* - pad_t),
pad_t = pad h / |d|, and the mirror image for far'.  A walk that accumulates t += dt does not meet it.
"""

import torch

R = 257
PADS = (0.0, 0.5, 2.0)
AMBIGUOUS_CAP = 0.02
U = 2.0 ** -24


def _hollow_shell(n=16):
    c = (torch.arange(n, dtype=torch.float64) + 0.5) * (2.0 / n) - 1.0
    z, y, x = torch.meshgrid(c, c, c, indexing="ij")
    r = (x * x + y * y + z * z).sqrt()
    return ((r > 0.45) & (r < 0.7)).to(torch.float32)[None]


def _random_scaffold(gen):
    u = torch.rand(2, 5, 6, 7, generator=gen)
    v = torch.where(torch.rand(2, 5, 6, 7, generator=gen) < 0.5, 0.5, 1.0)
    return torch.where(u < 0.25, v, torch.zeros(())).to(torch.float32)


SCAFFOLDS = {
    "random_2x5x6x7": lambda gen: _random_scaffold(gen),
    "one_cell_full": lambda gen: torch.ones(1, 1, 1, 1),
    "one_cell_empty": lambda gen: torch.zeros(1, 1, 1, 1),
    "alternating_1x1x1x9": lambda gen: (torch.arange(9) % 2 == 0).to(torch.float32).reshape(1, 1, 1, 9),
    "ones_8": lambda gen: torch.ones(1, 8, 8, 8),
    "zeros_8": lambda gen: torch.zeros(1, 8, 8, 8),
    "shell_16": lambda gen: _hollow_shell(16),
    "box": lambda gen: None,
}
SEEDS = {name: 1000 + 17 * i for i, name in enumerate(SCAFFOLDS)}
CASE_NAMES = tuple(SCAFFOLDS)


def _unit(n, gen):
    v = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    return v / v.norm(dim=-1, keepdim=True)


def _cell_points(shape, cells, gen, margin=0.05):
    """points inside the given cells [n, 4] (b, z, y, x), at least `margin` of a cell from every face"""
    _, D, H, W = shape
    u = margin + (1.0 - 2.0 * margin) * torch.rand(cells.shape[0], 3, generator=gen, dtype=torch.float64)
    n = torch.tensor([W, H, D], dtype=torch.float64)
    idx = cells[:, [3, 2, 1]].to(torch.float64)
    return (idx + u) * (2.0 / n) - 1.0


def _rays(scaffold, gen):
    shape = (1, 1, 1, 1) if scaffold is None else tuple(scaffold.shape)
    B, D, H, W = shape
    occ = torch.ones(shape) if scaffold is None else scaffold
    occupied = (occ != 0).nonzero()
    all_cells = torch.ones(shape).nonzero()

    def pick(cells, n):
        src = cells if cells.shape[0] > 0 else all_cells
        return src[torch.randint(0, src.shape[0], (n,), generator=gen)]

    o = torch.zeros(R, 3, dtype=torch.float64)
    d = torch.zeros(R, 3, dtype=torch.float64)
    near = torch.zeros(R, dtype=torch.float64)
    far = torch.zeros(R, dtype=torch.float64)
    gi = torch.randint(0, B, (R,), generator=gen)
    kind = [""] * R
    pos = [0]

    def take(n, name):
        s = slice(pos[0], pos[0] + n)
        for i in range(s.start, s.stop):
            kind[i] = name
        pos[0] += n
        return s

    def aimed(s, target, dist_lo=1.9, dist_hi=3.2):
        """origins on a sphere outside the box, directions towards `target` (unit length; scaled at the end)"""
        n = s.stop - s.start
        o[s] = _unit(n, gen) * (dist_lo + (dist_hi - dist_lo) * torch.rand(n, 1, generator=gen, dtype=torch.float64))
        v = target - o[s]
        d[s] = v / v.norm(dim=-1, keepdim=True)
        return v.norm(dim=-1)

    def box_points(n, scale=0.9):
        return (torch.rand(n, 3, generator=gen, dtype=torch.float64) * 2.0 - 1.0) * scale

    # generic rays from outside through the box
    s = take(74, "generic")
    aimed(s, box_points(74))
    near[s], far[s] = 0.05, 6.0
    # rays that miss the box
    s = take(16, "miss_box")
    n = 16
    o[s] = _unit(n, gen) * 3.0
    t = _unit(n, gen)
    d[s] = torch.nn.functional.normalize(torch.cross(o[s], t, dim=-1), dim=-1)  # perpendicular to the origin: passes the box at distance 3
    near[s], far[s] = 0.0, 8.0
    # near inside the box
    s = take(24, "near_inside")
    dist = aimed(s, box_points(24, 0.6))
    near[s], far[s] = dist, 7.0
    # far before the box
    s = take(16, "far_before")
    dist = aimed(s, box_points(16, 0.5), dist_lo=2.6)  # (the far end stays outside the box's circumsphere)
    near[s], far[s] = 0.0, 0.2 * dist
    # far inside the object: the ray ends in the middle of an occupied cell
    s = take(24, "far_inside_object")
    cells = pick(occupied, 24)
    gi[s] = cells[:, 0]
    dist = aimed(s, _cell_points(shape, cells, gen, 0.3))
    near[s], far[s] = 0.1, dist
    # origin inside an occupied cell
    s = take(24, "origin_in_occupied")
    cells = pick(occupied, 24)
    gi[s] = cells[:, 0]
    o[s] = _cell_points(shape, cells, gen, 0.2)
    d[s] = _unit(24, gen)
    near[s], far[s] = 0.0, 5.0
    # origin inside the box
    s = take(24, "origin_in_box")
    o[s] = box_points(24, 0.95)
    d[s] = _unit(24, gen)
    near[s], far[s] = 0.0, 5.0
    # far < near: both ends in front of the box (module docstring)
    s = take(16, "far_lt_near")
    aimed(s, box_points(16, 0.5), dist_lo=3.0, dist_hi=3.5)
    near[s], far[s] = 0.9, 0.4
    # zero direction components: the origin's coordinates on those axes sit inside a cell, 0.05 of a cell from its faces
    for nz, cnt in ((1, 12), (2, 9), (3, 4)):
        s = take(cnt, f"zero_{nz}")
        cells = torch.cat([pick(occupied, cnt // 2), pick(all_cells, cnt - cnt // 2)])  # half of them through an occupied cell
        gi[s] = cells[:, 0]
        p = _cell_points(shape, cells, gen, 0.05)
        v = _unit(cnt, gen)
        for j in range(cnt):
            axes = torch.randperm(3, generator=gen)[:nz]
            v[j, axes] = 0.0
            if nz < 3:
                v[j] = v[j] / v[j].norm()
        back = 0.5 + 2.5 * torch.rand(cnt, 1, generator=gen, dtype=torch.float64)
        if nz == 1 and cnt > 2:
            p[:2, 0] += 2.5  # two of them pass beside the box ...
            v[:2, 0] = 0.0   # ... along a zero component
            v[:2] = torch.nn.functional.normalize(v[:2] + torch.tensor([0.0, 0.3, 0.2], dtype=torch.float64), dim=-1)
        o[s] = p - back * v
        d[s] = v
        near[s], far[s] = 0.0, 6.0
    # ill-conditioned: one component tiny but not zero
    s = take(8, "ill_conditioned")
    aimed(s, box_points(8, 0.8))
    for j in range(8):
        a = j % 3
        i = s.start + j
        big = d[i].abs().max() if d[i].abs().argmax() != a else d[i].abs().sort().values[1]
        d[i, a] = (1.0 if j % 2 else -1.0) * big * (10.0 ** -(3.5 + 0.5 * (j // 2)))
    near[s], far[s] = 0.05, 6.0
    # NaN / Inf entries
    s = take(4, "non_finite")
    aimed(s, box_points(4))
    near[s], far[s] = 0.05, 6.0
    # grid_idx out of range
    s = take(2, "grid_idx_out_of_range")
    aimed(s, box_points(2, 0.3))
    near[s], far[s] = 0.05, 6.0
    assert pos[0] == R
    # lengths 0.3 / 1 / 3 in turn (zero directions stay zero)
    scale = torch.tensor([0.3, 1.0, 3.0], dtype=torch.float64)[torch.arange(R) % 3]
    d = d * scale[:, None]
    near, far = near / scale, far / scale
    o32, d32, n32, f32 = (t.to(torch.float32) for t in (o, d, near, far))
    i0 = kind.index("non_finite")
    o32[i0, 1] = float("nan")
    d32[i0 + 1, 2] = float("inf")
    n32[i0 + 2] = float("nan")
    f32[i0 + 3] = float("inf")
    gi = gi.to(torch.int32)
    i0 = kind.index("grid_idx_out_of_range")
    gi[i0] = -1
    gi[i0 + 1] = B if scaffold is not None else -7  # (without a scaffold every index >= 0 names the one box)
    # a zero component keeps its origin coordinate away from the faces also after the cast to fp32 (0.05 of a cell >> 1 ulp)
    return o32, d32, n32, f32, gi, kind


def oracle(scaffold, o, d, near, far, gi):
    """fp64 brute force (module docstring) -> dict of [R] tensors: hit, near_star, far_star, measure, nonempty, ambiguous, h"""
    shape = (1, 1, 1, 1) if scaffold is None else tuple(scaffold.shape)
    B, D, H, W = shape
    occ = torch.ones(shape) if scaffold is None else scaffold
    h = 2.0 / max(D, H, W)
    o, d, near, far = (t.to(torch.float64) for t in (o, d, near, far))
    n_r = o.shape[0]
    out = {k: torch.zeros(n_r, dtype=torch.float64) for k in ("near_star", "far_star", "measure")}
    hit = torch.zeros(n_r, dtype=torch.bool)
    nonempty = torch.zeros(n_r, dtype=torch.bool)
    ambiguous = torch.zeros(n_r, dtype=torch.bool)
    inf = float("inf")
    for r in range(n_r):
        b = int(gi[r])
        vals = torch.cat([o[r], d[r], near[r:r + 1], far[r:r + 1]])
        if not bool(torch.isfinite(vals).all()) or b < 0 or b >= B or far[r] < near[r]:
            continue
        cells = (occ[b] != 0).nonzero().to(torch.float64)  # (z, y, x)
        if cells.shape[0] == 0:
            continue
        lo = torch.full((cells.shape[0],), -inf, dtype=torch.float64)
        hi = torch.full((cells.shape[0],), inf, dtype=torch.float64)
        inside = torch.ones(cells.shape[0], dtype=torch.bool)
        for a, (n, col) in enumerate(((W, 2), (H, 1), (D, 0))):
            p0 = -1.0 + 2.0 * cells[:, col] / n
            p1 = -1.0 + 2.0 * (cells[:, col] + 1.0) / n
            if d[r, a] == 0:
                inside &= (p0 <= o[r, a]) & (o[r, a] <= p1)
            else:
                t0, t1 = (p0 - o[r, a]) / d[r, a], (p1 - o[r, a]) / d[r, a]
                lo = torch.maximum(lo, torch.minimum(t0, t1))
                hi = torch.minimum(hi, torch.maximum(t0, t1))
        cell_ok = inside & (lo <= hi)
        lo, hi = lo[cell_ok], hi[cell_ok]
        span = float(far[r] - near[r])
        if lo.numel() and span > 0:
            ends = torch.cat([lo, hi])
            ends = ends[torch.isfinite(ends)]
            if ends.numel() and bool((((ends - near[r]).abs() <= 1e-5 * span) | ((ends - far[r]).abs() <= 1e-5 * span)).any()):
                ambiguous[r] = True
        lo, hi = torch.clamp(lo, min=float(near[r])), torch.clamp(hi, max=float(far[r]))
        keep = lo <= hi
        lo, hi = lo[keep], hi[keep]
        if lo.numel() == 0:
            continue
        nonempty[r] = True
        order = torch.argsort(lo)
        lo, hi = lo[order], hi[order]
        reach = torch.cummax(hi, 0).values
        start = torch.maximum(lo, torch.cat([lo[:1], reach[:-1]]))  # the part of each interval the earlier ones do not cover
        m = float(torch.clamp(reach - start, min=0.0).sum())
        out["near_star"][r], out["far_star"][r], out["measure"][r] = float(lo.min()), float(hi.max()), m
        hit[r] = m > 0
        dn = float(d[r].norm())
        if dn > 0 and m < 1e-4 * h / dn:  # (a ray that does not move has the whole [near, far] or nothing)
            ambiguous[r] = True
    out.update(hit=hit, nonempty=nonempty, ambiguous=ambiguous, h=h)
    return out


_CASES = {}


def case(name):
    """the seeded case `name`: dict with scaffold (or None), o, d, near, far, grid_idx (fp32 / int32 CPU tensors), kind (list of
    strings), oracle (dict of `oracle`), built once and shared -- nobody writes to it"""
    if name not in _CASES:
        gen = torch.Generator().manual_seed(SEEDS[name])
        scaffold = SCAFFOLDS[name](gen)
        o, d, near, far, gi, kind = _rays(scaffold, gen)
        _CASES[name] = dict(name=name, scaffold=scaffold, o=o, d=d, near=near, far=far, grid_idx=gi, kind=kind,
                            oracle=oracle(scaffold, o, d, near, far, gi))
    return _CASES[name]


# ---------------------------------------------------------------------------------------------------------------------------
# Face gliders: rays that run along a cell face within rounding and END (or begin) inside the box.  One coordinate lies 0 .. 3 ulp
# from a plane of the cell tiling and moves by 1e-6 .. 1e-10 of the largest component, so the exact ray stays on one side of the face
# for its whole span while the Renderer's fp32 point (and its round-half-even index) may sit on the other.  They are ambiguous by
# nature: they take part in the conservativeness and exact-miss checks only, and the 2 % cap of the cases above -- a condition on
# THEIR rays -- does not count them.
# ---------------------------------------------------------------------------------------------------------------------------
GLIDER_R = 252
GLIDER_SCAFFOLDS = {
    "glide_1x1x1x4": lambda gen: torch.tensor([0.0, 0.0, 1.0, 1.0]).reshape(1, 1, 1, 4),
    "glide_alternating_1x1x1x9": SCAFFOLDS["alternating_1x1x1x9"],
    "glide_random_2x5x6x7": SCAFFOLDS["random_2x5x6x7"],
    "glide_shell_16": SCAFFOLDS["shell_16"],
    "glide_ones_1x3x2x5": lambda gen: torch.ones(1, 3, 2, 5),  # (occupied up to the faces of the box: a ray gliding on one is seen)
}
GLIDER_NAMES = tuple(GLIDER_SCAFFOLDS)
GLIDER_SEEDS = {name: 5000 + 13 * i for i, name in enumerate(GLIDER_SCAFFOLDS)}


def _glider_rays(scaffold, gen):
    B, D, H, W = scaffold.shape
    n_axis = (W, H, D)
    n = GLIDER_R
    o = torch.zeros(n, 3, dtype=torch.float32)
    d = torch.zeros(n, 3, dtype=torch.float32)
    near = torch.zeros(n, dtype=torch.float32)
    far = torch.zeros(n, dtype=torch.float32)
    gi = torch.randint(0, B, (n,), generator=gen).to(torch.int32)
    kind = []
    for i in range(n):
        a = i % 3
        size = n_axis[a]
        p = int(torch.randint(0, size + 1, (1,), generator=gen))  # a plane of the tiling, the box's faces included
        plane = torch.tensor((2 * p - size) / size, dtype=torch.float32)
        k = (i // 3) % 7 - 3  # -3 .. 3 ulp off the plane
        for _ in range(abs(k)):
            plane = torch.nextafter(plane, torch.tensor(2.0 if k > 0 else -2.0))
        # the other two coordinates: from outside the box (or, every fourth ray, from inside it) through a point inside
        tgt = (torch.rand(3, generator=gen) * 2.0 - 1.0) * 0.8
        src = _unit(1, gen)[0].to(torch.float32) * (2.0 + float(torch.rand(1, generator=gen)))
        if i % 4 == 3:
            src = (torch.rand(3, generator=gen) * 2.0 - 1.0) * 0.9
        v = tgt - src
        v[a] = 0.0
        v = v / v.norm()
        dist = float((tgt - src)[[j for j in range(3) if j != a]].norm())
        v[a] = (1.0 if (i // 5) % 2 else -1.0) * float(v.abs().max()) * 10.0 ** -(6 + (i // 7) % 5)
        src[a] = plane
        o[i], d[i] = src, v
        mode = ("far_inside", "near_inside", "both_inside")[(i // 3) % 3]
        if mode == "far_inside":
            near[i], far[i] = 0.0, dist
        elif mode == "near_inside":
            near[i], far[i] = dist, dist + 4.0
        else:  # a span shorter than a cell: the walk's first cell is its last
            near[i], far[i] = dist, dist + 0.4 * 2.0 / max(n_axis)
        kind.append("glider_" + mode)
    # the ray of the review that found the gap: x one rounding left of the plane x = 0, the span ends inside the box
    if tuple(scaffold.shape) == (1, 1, 1, 4):
        o[0], d[0] = torch.tensor([-2e-8, -2.0, 0.0]), torch.tensor([1e-10, 1.0, 0.0])
        near[0], far[0], gi[0] = 0.0, 2.5, 0
    scale = torch.tensor([0.3, 1.0, 3.0])[torch.arange(n) % 3]
    return o, d * scale[:, None], near / scale, far / scale, gi, kind


def glider_case(name):
    """the seeded face-glider case `name`: the dictionary of `case` without an oracle (nothing about these rays is compared to one)"""
    if name not in _CASES:
        gen = torch.Generator().manual_seed(GLIDER_SEEDS[name])
        scaffold = GLIDER_SCAFFOLDS[name](gen)
        o, d, near, far, gi, kind = _glider_rays(scaffold, gen)
        _CASES[name] = dict(name=name, scaffold=scaffold, o=o, d=d, near=near, far=far, grid_idx=gi, kind=kind)
    return _CASES[name]


def lin01(k):
    """torch.linspace(0, 1, k) in fp32: the Renderer's sample schedule (lin01 of lp_device.h follows it bit for bit)"""
    return torch.linspace(0.0, 1.0, k, dtype=torch.float32)


def lookup(c, k):
    """(depths [R, k] fp32, scaffold value at the Renderer's sample points [R, k]): depths near + lin01 * (far - near), points
    depth * d + o in fp32, looked up with the oracle's nearest-neighbour sampler.  Without a scaffold: the in-bounds mask.  Rays whose
    grid_idx is out of range have no scene to look up: their row is 0."""
    from oracle.lightplane_oracle import in_bounds, sample_scaffold_nearest
    depths = c["near"][:, None] + lin01(k)[None] * (c["far"] - c["near"])[:, None]
    pts = depths[..., None] * c["d"][:, None] + c["o"][:, None]
    pts = torch.where(torch.isfinite(pts), pts, torch.full_like(pts, 2.0))  # (a NaN / Inf point is outside the box: value 0)
    if c["scaffold"] is None:
        val = in_bounds(pts).to(torch.float32)
        val[c["grid_idx"] < 0] = 0.0
        return depths, val
    B = c["scaffold"].shape[0]
    in_range = (c["grid_idx"] >= 0) & (c["grid_idx"] < B)
    gi = torch.where(in_range, c["grid_idx"], torch.zeros_like(c["grid_idx"]))
    val = sample_scaffold_nearest(c["scaffold"], pts, gi)
    val = torch.nan_to_num(val, nan=0.0)
    val[~in_range] = 0.0
    return depths, val


def check_conservative(c, near_o, far_o, hit, ks=(2048, 7, 64, 128)):
    """every ray: no sample with a non-zero lookup outside [near', far'] (hit) or at all (miss); near <= near' <= far' <= far"""
    near, far = c["near"], c["far"]
    for k in ks:
        depths, val = lookup(c, k)
        nz = val != 0
        outside = nz & ((depths < near_o[:, None]) | (depths > far_o[:, None]))
        bad = (outside & hit[:, None]).any(dim=1)
        assert not bool(bad.any()), (c["name"], k, "occupied samples outside the clipped span of rays", bad.nonzero().flatten().tolist()[:8],
                                     [c["kind"][i] for i in bad.nonzero().flatten().tolist()[:8]])
        bad = (nz & ~hit[:, None]).any(dim=1)
        assert not bool(bad.any()), (c["name"], k, "occupied samples on missed rays", bad.nonzero().flatten().tolist()[:8],
                                     [c["kind"][i] for i in bad.nonzero().flatten().tolist()[:8]])
    ordered = torch.isfinite(near) & torch.isfinite(far) & (near <= far)
    ok = (near <= near_o) & (near_o <= far_o) & (far_o <= far)
    assert bool(ok[ordered].all()), (c["name"], "near <= near' <= far' <= far", (~ok & ordered).nonzero().flatten().tolist()[:8])


def check_misses(c, near_o, far_o, hit):
    """missed rays carry their input near / far bit for bit; NaN / Inf, far < near and out-of-range rays are misses"""
    miss = ~hit
    same = (near_o.view(torch.int32) == c["near"].view(torch.int32)) & (far_o.view(torch.int32) == c["far"].view(torch.int32))
    assert bool(same[miss].all()), (c["name"], (miss & ~same).nonzero().flatten().tolist()[:8])
    for i, kind in enumerate(c["kind"]):
        if kind in ("non_finite", "grid_idx_out_of_range", "far_lt_near", "miss_box", "far_before"):
            assert not bool(hit[i]), (c["name"], i, kind)


def tight_mask(c):
    """the rays of the tightness comparison: unambiguous, finite, every non-zero component |d_a| >= 1e-3 |d|_inf"""
    d = c["d"].to(torch.float64)
    dmax = d.abs().max(dim=1).values
    well = ((d == 0) | (d.abs() >= 1e-3 * dmax[:, None])).all(dim=1)
    finite = torch.isfinite(torch.cat([c["o"], c["d"], c["near"][:, None], c["far"][:, None]], dim=1)).all(dim=1)
    return well & finite & ~c["oracle"]["ambiguous"]


def check_tight(c, near_o, far_o, hit, pad):
    orc = c["oracle"]
    m = tight_mask(c)
    wrong = m & (hit != orc["hit"])
    assert not bool(wrong.any()), (c["name"], pad, "hit != hit64", wrong.nonzero().flatten().tolist()[:8],
                                   [c["kind"][i] for i in wrong.nonzero().flatten().tolist()[:8]])
    o, d, near, far = (c[k].to(torch.float64) for k in ("o", "d", "near", "far"))
    dn = d.norm(dim=1)
    q = torch.where(d != 0, (1.0 + o.abs()) / d.abs(), torch.zeros_like(d)).max(dim=1).values
    pad_t = torch.where(dn > 0, pad * orc["h"] / dn, torch.full_like(dn, float("inf")))
    exp_near = torch.maximum(near, orc["near_star"] - pad_t)
    exp_far = torch.minimum(far, orc["far_star"] + pad_t)
    sel = m & orc["hit"]
    worst = 0.0
    for i in sel.nonzero().flatten().tolist():
        tol_n = 16 * U * float(q[i]) + 4 * U * abs(float(exp_near[i]))
        tol_f = 16 * U * float(q[i]) + 4 * U * abs(float(exp_far[i]))
        gn, gf = float(near_o[i]), float(far_o[i])
        assert exp_near[i] - 2 * tol_n <= gn <= exp_near[i] + tol_n, (c["name"], pad, i, c["kind"][i], "near'", gn, float(exp_near[i]), tol_n)
        assert exp_far[i] - tol_f <= gf <= exp_far[i] + 2 * tol_f, (c["name"], pad, i, c["kind"][i], "far'", gf, float(exp_far[i]), tol_f)
        if tol_n > 0 and tol_f > 0:  # (a ray that does not move has expected == near / far exactly)
            worst = max(worst, (float(exp_near[i]) - gn) / tol_n, (gf - float(exp_far[i])) / tol_f)
    return int(sel.sum()), worst

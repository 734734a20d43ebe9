"""The scripted batches of tests/walk_cases.py without a GPU: that every case drives the walks through the transitions it is listed for and
the table as a whole through every one (the ledger), that no single contribution is small enough to hide behind the bar, that the fp32
oracle meets the fp64 oracle there, and what the suite's pinhole images and random rays reached until now."""
import numpy as np
import pytest
import torch

from oracle import lightplane_oracle as O
from tests import walk_cases as WC

F64 = torch.float64
BAR = 1e-4            # the project's bar: of the tensor's largest entry
HIDE_FACTOR = 4.0     # the smallest single contribution is at least this many bars
ORACLE_BAR = 2e-5     # fp32 oracle against fp64 oracle

FORWARD = WC.FORWARD_RAYS + WC.FORWARD_SAMPLES
_IDS = [f"{n}-c{C}-{form}" for n, C, form in FORWARD]

# what a case is listed for ("Walk transitions"): asserted for every launch of the case whose walk has the predicate
CARRIES = {
    "main": ["run_one_run_over_the_whole_wave", "run_every_lane_a_head", "run_heads_exactly_at_every_8th_lane", "run_all_dead_wave_sample",
             "run_ragged_last_wave", "run_ray_count_no_multiple_of_the_block_or_the_wave"] +
    [f"step_{a}_{s}_equal_validity" for a in "xyz" for s in ("plus", "minus")] + [f"step_of_2_along_{a}" for a in "xyz"] +
    [f"diag_{p}_{s}" for p in ("xy", "xz", "yz") for s in ("pp", "pm", "mp", "mm")] + ["diag_three_axes"] + WC._ENTRIES +
    ["window_iu_14_to_15", "window_iu_15_to_16", "window_lane_at_iu_minus_1", "window_lane_at_iu_last", "window_left_along_x_backward"],
    "main_mask": ["run_lane0_dead", "run_dead_lane_inside_a_run_of_one_cell", "step_across_the_low_border_validity_differs",
                  "step_across_the_high_border_validity_differs", "diag_shared_column_validity_differs"],
    "window_w2": ["window_base_at_minus_1", "window_lane_at_iu_last", "window_line_step_y_plus", "window_line_step_z_plus",
                  "window_line_step_because_the_entry_changed"],
    "window_w15": ["window_left_along_x_by_15_or_more", "window_line_step_together_with_leaving_x", "window_left_along_x_backward"],
    "window_w16": ["window_iu_14_to_15", "window_base_rule_iu_and_15_is_15_on_rebase", "window_left_along_x_by_15_or_more"],
    "window_w17": ["window_iu_14_to_15", "window_iu_15_to_16", "window_left_along_x_forward", "window_line_step_only_by_a_row_alias"],
    "window_w33": ["window_iu_14_to_15", "window_iu_15_to_16", "window_base_rule_iu_and_15_is_15_on_rebase", "window_line_step_y_minus",
                   "window_line_step_z_minus"],
    "transposed_s33": ["transposed_last_block_has_dead_lanes", "run_one_run_over_the_whole_wave", "run_heads_exactly_at_every_8th_lane"] +
    [f"diag_{p}_{s}" for p in ("xy", "xz", "yz") for s in ("pp", "pm", "mp", "mm")] + ["diag_three_axes"] + [f"step_of_2_along_{a}" for a in "xyz"],
    "transposed_s40_mask": ["transposed_last_block_has_dead_lanes", "step_across_the_low_border_validity_differs",
                            "step_across_the_high_border_validity_differs", "diag_shared_column_validity_differs"],
    "transposed_w33_s40": ["window_iu_14_to_15", "window_iu_15_to_16"],
}
for _a in "xyz":
    CARRIES[f"long_{_a}1022"] = [f"packable_edge_1022_along_{_a}", f"step_{_a}_plus_equal_validity"]
    for _n in (1023, 1500):
        CARRIES[f"long_{_a}{_n}"] = [f"unpackable_axis_{_a}", f"unpackable_unit_step_along_{_a}_not_carried"]
    CARRIES[f"long_{_a}1500"] += [f"unpackable_lane_beyond_cell_1023_along_{_a}"]
    CARRIES[f"transposed_long_{_a}1500"] = [f"unpackable_axis_{_a}", f"unpackable_lane_beyond_cell_1023_along_{_a}",
                                             f"unpackable_unit_step_along_{_a}_not_carried"]


def _known(walks):
    out = set()
    for k in walks:
        out |= set(WC.REQUIRED[k])
    return out


@pytest.mark.parametrize("name,C,form", FORWARD, ids=_IDS)
def test_every_launch_reaches_what_its_case_is_listed_for(name, C, form):
    case = WC.CASES[name]
    led = WC.ledger_of(case, C, form)
    keys = WC.walk_keys(C, form, case.order)
    want = [p for p in CARRIES[name] if p in _known(keys) and (form != "triplane" or p.startswith("plane"))]
    missed = [p for p in want if led[p] == 0]
    print(f"walk ledger {name} C={C} {form} [{', '.join(keys)}]: {len(led.reached())} predicates reached, {len(want)} listed")
    assert not missed, f"{name} C={C} {form}: listed but not reached: {missed}"


def test_the_table_reaches_every_transition_of_every_walk():
    union = {}
    for name, C, form in FORWARD:
        case = WC.CASES[name]
        led = WC.ledger_of(case, C, form)
        for k in WC.walk_keys(C, form, case.order):
            union.setdefault(k, WC.Ledger()).update(led)
    union["backward"] = WC.Ledger()
    for name, C, row in WC.BACKWARD:
        union["backward"].update(WC.backward_ledger_of(WC.CASES[name], C, row))
    assert set(union) == set(WC.REQUIRED)
    for k, req in WC.REQUIRED.items():
        missed = [p for p in req if union[k][p] == 0]
        assert not missed, f"walk {k}: no case reaches {missed}"
    widths = {WC.CASES[n].base[3] for n in WC.WINDOW_CASES}
    assert widths >= set(WC.GRID_WIDTHS_REQUIRED)
    for ax in range(3):   # (B, D, H, W): x is the last
        assert {WC.CASES[n].base[3 - ax] for n in WC.LONG_CASES if n.startswith(f"long_{WC.AXES[ax]}")} == set(WC.LONG_AXES_REQUIRED)
    for n in WC.LONG_CASES:
        b = WC.CASES[n].base
        assert sorted(b[1:])[:2] <= [3, 3] and b[0] * b[1] * b[2] * b[3] <= 20000, n


def test_the_ledger_restates_patch_ray_index_as_a_bijection():
    for n, w in ((64, 8), (48, 8), (50, 8), (7, 8), (96, 3)):
        idx = WC.patch_ray_index(np.arange(n), n, w)
        assert sorted(idx.tolist()) == list(range(n))
    assert WC.patch_ray_index(np.arange(8), 64, 8).tolist() == [0, 8, 16, 24, 25, 17, 9, 1]   # a snake down and up two columns


def _contributions(rays64, sizes, cfg):
    """per output grid (smallest single contribution to the feature sums, to the weight sums) over every live tap"""
    points = O._splatter_points(rays64, cfg["num_samples"], 0, False, 1e-5)
    mask = O.in_bounds(points) if cfg["mask_out_of_bounds_samples"] else torch.ones(points.shape[:-1], dtype=torch.bool)
    emin = rays64.encoding.abs().min(dim=1).values[:, None]
    out = []
    for gs in sizes:
        wmin, fmin = float("inf"), float("inf")
        for _, w, valid in O._corner_setup(points, gs, O._unnormalize_splatter):
            live = valid & mask
            if live.any():
                wmin = min(wmin, float(w[live].min()))
                fmin = min(fmin, float((w * emin)[live].min()))
        out.append((fmin, wmin))
    return out


@pytest.mark.parametrize("name,C,form", FORWARD, ids=_IDS)
def test_no_contribution_hides_and_the_oracles_agree(name, C, form):
    """Smallest single contribution >= 4 bars per output tensor (one dropped, doubled or misplaced contribution cannot pass); the fp32
    oracle within 2e-5 of the fp64 oracle on the feature sums, the weight sums and the normalised output; identical cells in both
    geometries."""
    case = WC.CASES[name]
    rays, cfg, sizes = WC.build_rays(case, C), WC.splat_cfg(case), WC.grid_sizes(case, C, form)
    r64 = WC.rays_as(rays, F64)
    s64, s32 = O.splatter_sums(r64, sizes, **cfg), O.splatter_sums(rays, sizes, **cfg)
    n64, n32 = O.lightplane_splatter_naive(r64, sizes, **cfg), O.lightplane_splatter_naive(rays, sizes, **cfg)
    for g, ((fmin, wmin), (f64, w64), (f32, w32)) in enumerate(zip(_contributions(r64, sizes, cfg), s64, s32)):
        fbar, wbar = BAR * float(f64.abs().max()), BAR * float(w64.abs().max())
        ef = float((f32.double() - f64).abs().max()) / float(f64.abs().max())
        ew = float((w32.double() - w64).abs().max()) / float(w64.abs().max())
        en = float((n32[g].double() - n64[g]).abs().max()) / float(n64[g].abs().max())
        print(f"walk case {name} C={C} {form} grid {g}: smallest contribution {fmin:.4g} = {fmin / fbar:.1f} bars (features), {wmin:.4g} = "
              f"{wmin / wbar:.1f} bars (weights); fp32 oracle from fp64: {ef:.2e} features, {ew:.2e} weights, {en:.2e} normalised")
        assert fmin >= HIDE_FACTOR * fbar, f"{name} grid {g}: a feature contribution of {fmin:.3g} against a bar of {fbar:.3g}"
        assert wmin >= HIDE_FACTOR * wbar, f"{name} grid {g}: a weight contribution of {wmin:.3g} against a bar of {wbar:.3g}"
        assert max(ef, ew, en) <= ORACLE_BAR, f"{name} grid {g}: fp32 oracle {ef:.2e} / {ew:.2e} / {en:.2e} from the fp64 oracle"
        assert torch.equal(f32.abs().sum(dim=1) != 0, f64.abs().sum(dim=1) != 0) and torch.equal(w32 != 0, w64 != 0)
    B, D, H, W = case.base
    i32, l32 = WC.cells_of(rays, cfg["num_samples"], case.mask, torch.float32, sizes_xyz=(W, H, D))
    i64, l64 = WC.cells_of(rays, cfg["num_samples"], case.mask, F64, sizes_xyz=(W, H, D))
    assert all(np.array_equal(a, b) for a, b in zip(i32, i64)) and np.array_equal(l32, l64), f"{name}: fp32 and fp64 geometry disagree on a cell"


@pytest.mark.parametrize("name,C,row", WC.BACKWARD, ids=[f"{n}-c{C}-row{r}" for n, C, r in WC.BACKWARD])
def test_backward_launches_reach_their_transitions(name, C, row):
    led = WC.backward_ledger_of(WC.CASES[name], C, row)
    want = ["backward_run_of_several_rays_reads_once", "backward_head_reads_again"]
    if row:
        want += ["backward_patch_order_2x4_pixels", "backward_patch_image_height_multiple_of_4" if name == "patch_8x8" else "backward_patch_tail_keeps_scanline_order"]
    elif name.startswith("transposed"):
        want += ["backward_several_segments"]
    else:
        want += ["backward_one_segment", "backward_ragged_last_wave", "backward_lane0_dead", "backward_head_in_the_other_entry"]
    assert not [p for p in want if led[p] == 0], (name, dict(led))


# ---- what the suite reached until now ---------------------------------------------------------------------------------------------------------
def _old_inputs():
    """(tag, rays, voxel base (B, D, H, W), cfg) of every voxel splat of test_splatter_coherent_image (SPLATS x IMAGES, masked),
    test_splatter_random_cameras and test_splatter_walk_touched_cells_equal_oracle"""
    from tests.synth import cat_rays, pinhole_rays
    from tests.test_gpu_coherent import IMAGES, SPLATS, coherent_splatter_inputs
    from tests.test_gpu_config_scale import SPLAT_INDEX_CASES
    for name, (base, tri, _) in SPLATS.items():
        if tri:
            continue
        for image in IMAGES:
            d = coherent_splatter_inputs(name, image)
            yield f"coherent {name}/{image}", d["rays"], base[:4], base[4], d["cfg"]
    for seed in range(12):
        gen = torch.Generator().manual_seed(1000 + seed)
        rnd = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=gen))  # noqa: E731
        C = (32, 64, 16, 32)[seed % 4]
        batch = 1 + (seed % 3 == 2)
        base = (batch, rnd(10, 26), rnd(10, 26), rnd(10, 26))
        parts = [pinhole_rays(40, 56, grid_idx=b, azimuth_deg=float(torch.rand(1, generator=gen)) * 360.0,
                              elevation_deg=float(torch.rand(1, generator=gen)) * 120.0 - 60.0) for b in range(batch)]
        rays = parts[0] if batch == 1 else cat_rays(parts)
        torch.rand(rays.n_rays, C, generator=gen)
        cfg = dict(num_samples=rnd(20, 45), num_samples_inf=0, mask_out_of_bounds_samples=bool(seed & 1), contract_coords=False)
        yield f"random camera {seed}", rays, base, C, cfg
    for name, (base, tri, H, W, az, el, S, mask) in SPLAT_INDEX_CASES.items():
        if tri:
            continue
        parts = [pinhole_rays(H, W, cam_dist=2.2, grid_idx=b, azimuth_deg=az + 50.0 * b, elevation_deg=el) for b in range(base[0])]
        rays = parts[0] if len(parts) == 1 else cat_rays(parts)
        yield f"index case {name}", rays, base[:4], base[4], dict(num_samples=S, num_samples_inf=0, mask_out_of_bounds_samples=mask, contract_coords=False)


def test_what_the_pinhole_images_of_the_suite_reached():
    """The ledger over the voxel splats of the three pinhole-image tests: never two batch entries in one wave (the batch boundary of
    every two-entry image falls on a wave boundary), no axis above 1 022 cells, none of the grid widths 2 / 15 / 17 / 33; which
    window edges and which other predicates they happened to reach is printed and recorded in DESIGN.md."""
    total = {}
    widths = set()
    for tag, rays, base, C, cfg in _old_inputs():
        dealing, walk = WC.forward_walks(C, "voxel", "rays")
        rays.encoding = torch.zeros(rays.n_rays, 1)    # (the ledger reads the geometry alone)
        L = WC.voxel_lanes(rays, cfg, base, dealing)
        led = WC.classify_window(L, WC.classify_voxel(L, walk))
        total.setdefault(walk, WC.Ledger()).update(led)
        widths.add(base[3])
        assert max(base[1:]) <= WC.PACK_MAX, tag
        entry = [p for p in led.reached() if p.startswith("entry_") or p == "alias_row_last_corner_against_next_entry"
                 or p.endswith("the_entry_changed") or p.endswith("other_entry_refused") or p.endswith("refused_by_row_delta")]
        assert not entry, f"{tag}: two batch entries in one wave after all: {entry}"
        assert not (L.b.min(axis=1) != L.b.max(axis=1)).any(), tag
    print(f"old inputs: grid widths along x {sorted(widths)}")
    # (one old grid is 16 cells wide -- SPLATS["voxel18_c64"] -- and the window edges 14 -> 15 and 15 -> 16 ARE reached, by the 18 .. 26
    # cell grids: thousands of times, but by whatever ray happens to sit there; widths 2, 15, 17 and 33 are absent)
    assert not widths & {2, 15, 17, 33}, widths
    assert not any(p.startswith(("unpackable", "packable_edge")) for led in total.values() for p in led.reached())
    for walk, led in total.items():
        key = {"one_axis": ["one_axis", "window"], "two_axis": ["two_axis", "window"]}[walk]
        req = [p for k in key for p in WC.REQUIRED[k]]
        missed = sorted(set(p for p in req if led[p] == 0))
        print(f"old inputs, {walk} walk: {len(set(req)) - len(missed)} of {len(set(req))} predicates reached; never reached: {missed}")
        edges = {p: led[p] for p in ("window_iu_14_to_15", "window_iu_15_to_16", "window_lane_at_iu_minus_1", "window_lane_at_iu_last")}
        print(f"old inputs, {walk} walk: window edges {edges}")
        assert missed, "the old inputs reach everything: the scripted cases would add nothing"


# ---- the Renderer carriers: the same walk in the Renderer's convention ---------------------------------------------------------------------------
def _renderer_carriers():
    from tests.test_gpu_walk_transitions import RENDERER
    return RENDERER


@pytest.mark.parametrize("name,C,order", _renderer_carriers(), ids=[f"{n}-c{C}-{o}" for n, C, o in _renderer_carriers()])
def test_renderer_carriers_take_the_one_axis_walk_through_its_transitions(name, C, order):
    """The ledger of a Renderer carrier is built in the Renderer's un-normalisation and held against ``oracle.renderer_corner_indices``
    row by row; the tuned backward deals 32 rays (or 32 samples of one ray) to a wave and scatters with ``splat_walk_vox``"""
    import lightplane_amd as lp
    from tests.test_gpu_walk_transitions import renderer_inputs
    case = WC.CASES[name]
    d = renderer_inputs(name, C)
    assert lp.kernel_family(d["rays"], d["grids"], d["decoder"]) == 1
    B, D, H, W = case.base
    S = case.num_samples
    idx, _ = WC.cells_of(d["rays"], S, False, torch.float32, O._unnormalize_renderer, (W, H, D))
    rows = O.renderer_corner_indices(d["rays"], d["sizes"], S)[0].numpy()
    row0 = d["rays"].grid_idx.numpy()[:, None] * (D * H * W) + (idx[2] * H + idx[1]) * W + idx[0]
    for k in range(8):
        ux, uy, uz = k & 1, (k >> 1) & 1, k >> 2
        ok = np.ones(row0.shape, dtype=bool)
        for a, u, n in ((idx[0], ux, W), (idx[1], uy, H), (idx[2], uz, D)):
            ok &= (a + u >= 0) & (a + u <= n - 1)
        assert np.array_equal(rows[..., k], np.where(ok, row0 + ux + uy * W + uz * H * W, -1)), f"{name}: corner {k}"
    cfg = dict(num_samples=S, mask_out_of_bounds_samples=case.mask)
    L = WC.voxel_lanes(d["rays"], cfg, case.base, "samples" if order == "samples" else "rays32", unnormalize=O._unnormalize_renderer)
    led = WC.classify_voxel(L, "one_axis")
    want = [p for p in CARRIES[name] if p in WC.REQUIRED["one_axis_transposed" if order == "samples" else "one_axis"]
            and not p.startswith(("transposed_", "run_ray_count"))]   # (those two are facts of the launch, counted by ``ledger_of``)
    missed = [p for p in want if led[p] == 0]
    print(f"walk ledger Renderer {name} C={C} [{order}]: {len(led.reached())} predicates reached, {len(want)} listed")
    assert not missed, f"Renderer carrier {name}: listed but not reached: {missed}"
    i64, _ = WC.cells_of(d["rays"], S, False, F64, O._unnormalize_renderer, (W, H, D))
    assert all(np.array_equal(a, b) for a, b in zip(idx, i64))


# ---- the per-slot run loop: the launches that reach every site of it ------------------------------------------------------------------------------
def _assert_slot_branches(tag, row, ok, masked, fast_path):
    """One grid of one launch takes the branches of the per-slot run loop: a wave-sample that is a single live run (the fast path where
    the site has one), one of two or more runs and, under the out-of-bounds mask, a dead run directly between two live ones."""
    led = WC.classify_slot_runs(row, ok)
    print(f"slot-walk ledger {tag}{' (single-run fast path)' if fast_path else ''}: {dict(led)}")
    want = ["slot_single_live_run", "slot_several_runs"] + (["slot_dead_run_between_two_live_runs"] if masked else [])
    missed = [p for p in want if led[p] == 0]
    assert not missed, f"{tag}: not reached: {missed}"


def _renderer_plane_launches():
    from tests.test_gpu_walk_transitions import RENDERER_PLANES
    return RENDERER_PLANES


@pytest.mark.parametrize("name,C,order,form", _renderer_plane_launches(), ids=[f"{n}-c{C}-{o}-{f}" for n, C, o, f in _renderer_plane_launches()])
def test_renderer_plane_launches_take_the_branches_of_the_slot_walk(name, C, order, form):
    """The tuned backward on a canonical triplane (``scatter_triplane``: sentinel rows, per plane) and on [voxel, xy plane] (the tail of
    ``scatter_grid`` on the plane: rows and validity bits), in the Renderer's un-normalisation, 32 rays or 32 samples of a ray per wave"""
    import lightplane_amd as lp
    from tests.test_gpu_walk_transitions import renderer_inputs
    case = WC.CASES[name]
    d = renderer_inputs(name, C, form)
    assert lp.kernel_family(d["rays"], d["grids"], d["decoder"]) == 1
    cfg = dict(num_samples=case.num_samples, mask_out_of_bounds_samples=case.mask)
    dealing = "samples" if order == "samples" else "rays32"
    tag = f"Renderer {name} C={C} [{order}] {form}"
    if form == "triplane":
        for g, row in enumerate(WC.triplane_sentinel_rows(d["rays"], cfg, case.base, dealing)):
            _assert_slot_branches(f"{tag} plane {g}", row, row >= 0, case.mask, True)
    else:
        B, D, H, W = case.base
        L = WC.plane_lanes(d["rays"], cfg, (B, 1, H, W), dealing, unnormalize=O._unnormalize_renderer)
        _assert_slot_branches(f"{tag} xy plane", WC.plane_rows(L), L.ok, case.mask, True)


@pytest.mark.parametrize("name", ["main", "main_mask"])
def test_mlp_splatter_plane_launches_take_the_branches_of_the_slot_walk(name):
    """The MLP-Splatter with [voxel, xy plane] outputs: its forward walks the plane slot by slot from the LDS tile (Splatter convention, no
    fast path), its backward scatters the input-grid gradient with the two-pass form of ``scatter_grid`` (Renderer convention, voxel grid)"""
    from tests.test_gpu_walk_transitions import MLP_IN_BASE
    case = WC.CASES[name]
    rays, cfg = WC.build_rays(case, 32), WC.splat_cfg(case)
    B, D, H, W = case.base
    L = WC.plane_lanes(rays, cfg, (B, 1, H, W), "rays32")
    _assert_slot_branches(f"MLP-Splatter {name} forward, xy plane", WC.plane_rows(L), L.ok, case.mask, False)
    L = WC.voxel_lanes(rays, cfg, (B,) + MLP_IN_BASE, "rays32", unnormalize=O._unnormalize_renderer)
    _assert_slot_branches(f"MLP-Splatter {name} backward, voxel input grid", WC._rows(L), L.ok, case.mask, True)

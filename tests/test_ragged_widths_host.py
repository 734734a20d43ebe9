"""CPU tests of the ragged-width tables (tests/ragged_cases.py): the branch ledger is covered and every case adds to it, every Renderer
case stays on the shape-generic kernels, every case is well conditioned for the oracle (so the GPU tests' 1e-4 is never strained by the
reference arithmetic), and what the ABI does not take at these widths is refused on the host, before a launch."""
import copy
import ctypes

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib, grids, params
from lightplane_amd.modules import _fused_embedding_supported
from lightplane_amd.renderer import relu_dump_words
from oracle import lightplane_oracle as O
from tests import ragged_cases as R

ORACLE_TOL = 2e-5   # tests/test_oracle_golden.py REL_TOL: what the oracle itself is held to
F64 = torch.float64


# ---- the ledger -----------------------------------------------------------------------------------------------------------------------
def test_every_ledger_entry_is_reached_and_every_case_adds_one():
    """A kernel change that moves a threshold makes an entry unreachable (or a case redundant) and this fails: update the tables in
    tests/ragged_cases.py, do not delete the entry."""
    shapes = R.all_shapes()
    assert len({s.id for s in shapes}) == len(shapes)
    seen, report = set(), []
    for s in shapes:
        got = R.reached(s)
        new = [n for n in got if n not in seen]
        report.append(f"{s.id}: {len(got)} entries, new: {', '.join(new) or '-'}")
        assert got, f"{s.id} reaches no ledger entry"
        assert new, f"{s.id} reaches no ledger entry that an earlier case does not reach: {got}"
        seen |= set(got)
    print("\n".join(report))
    missing = [p.__name__ for p in R.LEDGER if p.__name__ not in seen]
    assert not missing, f"ledger entries no case reaches: {missing}"
    assert len({p.__name__ for p in R.LEDGER}) == len(R.LEDGER)
    for p in R.LEDGER:  # every predicate says which device lines it restates
        assert p.__doc__ and (".h:" in p.__doc__ or ".hip:" in p.__doc__), p.__name__


def test_the_case_tables_hold_what_they_promise():
    """The switches and counts the tables are to spread: every one appears at least once."""
    rc = R.RENDERER_CASES
    assert {c.n_rays for c in rc} == {1, 63, 65, 130}
    assert {c.grid_base[0] for c in rc} == {1, 2, 3}
    assert any(not c.is_triplane for c in rc) and any(c.is_triplane and not c.extra_voxel for c in rc) and any(c.extra_voxel for c in rc)
    assert any(c.mask_oob for c in rc) and any(c.contract for c in rc) and any(c.scaffold_size for c in rc) and any(c.two_grid for c in rc)
    assert any(not c.pad_color for c in rc)
    for c in rc:
        assert 5 <= c.num_samples <= 9 and max(c.grid_base[1:4]) <= 7, c.name
        d = c.build()
        assert d["cfg"]["num_samples_inf"] == 0
        assert all(max(g.shape[1:4]) <= 7 for g in d["grids"] + (d["color_grids"] or []))
    assert [c.dims for c in R.MLP_SPLATTER_CASES] == [(5, 20, 7), (33, 47, 24, 100), (12, 9, 3), (128, 128, 128)]
    sc = R.SPLATTER_CASES
    assert [c.out_base[-1] for c in sc] == [1, 3, 5, 20, 33, 100, 128]
    assert {c.n_rays for c in sc} == {1, 17, 130} and {c.is_triplane for c in sc} == {False, True}
    assert any(c.mask_oob for c in sc) and any(c.num_samples_inf > 0 for c in sc)
    assert R.EMBEDDING_CASES == [(3, 3, 257), (1, 1, 5), (0, 33, 64), (10, 85, 300)]


# ---- selection ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.RENDERER_CASES, ids=lambda c: c.name)
def test_renderer_cases_stay_on_the_shape_generic_kernels(case):
    """(``lp_renderer_kernel_family`` looks at shapes only: no GPU.)  The Shape the ledger reads is the library's own view of the case:
    its ReLU sites are the dump's."""
    d = case.build()
    assert lp.kernel_family(d["rays"], d["grids"], d["decoder"], color_grid=d["color_grids"], num_samples_inf=0) == 0
    assert lp.forward_kernel_family(d["rays"], d["grids"], d["decoder"], color_grid=d["color_grids"], num_samples_inf=0) == 0
    s = R.renderer_shape(case)
    assert s.total <= 1024 and s.stage_ld <= _lib.LP_MAX_WIDTH + 1
    assert s.n_params == d["decoder"].mlp_params.numel()
    if int(_lib.build_info().get("test_hooks", 0)):
        words = relu_dump_words(d["rays"], d["grids"], d["decoder"], color_grid=d["color_grids"])
        assert words == len(s.sites) * (-(-max(s.sites) // 32)) + 1, (words, s.sites)


@pytest.mark.parametrize("case", R.MLP_SPLATTER_CASES, ids=lambda c: c.name)
def test_mlp_splatter_cases_stay_on_the_shape_generic_kernels(case):
    from lightplane_amd.splatter import mlp_splatter_kernel_family
    d = case.build()
    assert mlp_splatter_kernel_family(d["out_sizes"], d["mlp"], d["in_sizes"], 0) == 0
    assert R.mlp_splatter_shape(case).n_params == d["mlp"].mlp_params.numel()


@pytest.mark.parametrize("case", R.SPLATTER_CASES, ids=lambda c: c.name)
def test_splatter_cases_take_the_lpr_cpl_kernels(case):
    a = _lib.LpSplatterArgs()
    a.out = _lib.make_grid_list(None, [grids.GridDesc(*case.out_base[:4], 0)], case.out_base[-1], 1)
    assert _lib.lib().lp_splatter_kernel_family(ctypes.byref(a)) == 0


# ---- conditioning: the bar is never the excuse ------------------------------------------------------------------------------------------
def _within(tag, a32, a64):
    scale = float(a64.abs().max())
    assert scale > 0, f"{tag}: the output is zero everywhere"
    err = float((a32.double() - a64).abs().max()) / scale
    print(f"{tag}: fp32 oracle vs fp64 oracle {err:.3e}")
    assert err <= ORACLE_TOL, f"{tag}: the fp32 and the fp64 oracle differ by {err:.3e} of the largest entry (bar {ORACLE_TOL:g}): change the seed"


def _rays_as(rays, dtype):
    r = copy.copy(rays)
    for f in ("directions", "origins", "near", "far", "encoding"):
        setattr(r, f, getattr(r, f).to(dtype))
    return r


@pytest.mark.parametrize("case", R.RENDERER_CASES, ids=lambda c: c.name)
def test_renderer_cases_are_well_conditioned(case):
    d = case.build()
    outs = {}
    with torch.no_grad():
        for dt in (torch.float32, F64):
            dec = copy.copy(d["decoder"])
            dec.mlp_params = dec.mlp_params.to(dt)
            cg = None if d["color_grids"] is None else [g.to(dt) for g in d["color_grids"]]
            sc = None if d["scaffold"] is None else d["scaffold"].to(dt)
            outs[dt] = O.lightplane_renderer_naive(_rays_as(d["rays"], dt), [g.to(dt) for g in d["grids"]], dec, scaffold=sc, color_grid=cg,
                                                   **d["cfg"])
    for nm, a, b in zip(("ray_length", "neg_log_t", "feature"), outs[torch.float32], outs[F64]):
        _within(f"{case.name} {nm}", a, b)
    # a real test: the rays see something, and not everything (no output saturates)
    nlt = outs[F64][1]
    assert float(nlt.max()) > 0.05 and float(nlt.median()) < 20.0, f"{case.name}: -log T in [{float(nlt.min()):.3g}, {float(nlt.max()):.3g}]"


@pytest.mark.parametrize("case", R.MLP_SPLATTER_CASES, ids=lambda c: c.name)
def test_mlp_splatter_cases_are_well_conditioned(case):
    d = case.build()
    outs = {}
    with torch.no_grad():
        for dt in (torch.float32, F64):
            mlp = copy.copy(d["mlp"])
            mlp.mlp_params = mlp.mlp_params.to(dt)
            outs[dt] = O.lightplane_mlp_splatter_naive(_rays_as(d["rays"], dt), d["out_sizes"], mlp, [g.to(dt) for g in d["in_grids"]], **d["cfg"])
    for k, (a, b) in enumerate(zip(outs[torch.float32], outs[F64])):
        _within(f"{case.name} out{k}", a, b)


@pytest.mark.parametrize("case", R.SPLATTER_CASES, ids=lambda c: c.name)
def test_splatter_cases_are_well_conditioned(case):
    d = case.build()
    with torch.no_grad():
        o32 = O.lightplane_splatter_naive(d["rays"], d["out_sizes"], **d["cfg"])
        o64 = O.lightplane_splatter_naive(_rays_as(d["rays"], F64), d["out_sizes"], **d["cfg"])
    for k, (a, b) in enumerate(zip(o32, o64)):
        _within(f"{case.name} out{k}", a, b)


# ---- refusals: errors in Python, not launches --------------------------------------------------------------------------------------------
FAKE = 0x7F0000010000  # 16-byte aligned "device pointers": every call below fails a host check before anything could dereference them


def _renderer_args(C, dims_t, dims_o, dims_c, color_chn=3, n_rays=1):
    a = _lib.LpRendererArgs()
    a.rays.n_rays, a.rays.encoding_dim = n_rays, dims_c[0]
    for k, f in enumerate(("directions", "origins", "grid_idx", "near_t", "far_t", "encoding")):
        setattr(a.rays, f, FAKE + 0x1000 * k)
    a.grid = _lib.make_grid_list(None, [grids.GridDesc(1, 4, 4, 4, 0)], C, 64)
    a.grid.data = FAKE + 0x10000
    a.march = _lib.make_march(8, 0, False, False, 1e-5)
    n = [params.mlp_numel(x) if len(x) > 1 else 0 for x in (dims_t, dims_o, dims_c)]
    a.trunk, a.opacity, a.color = _lib.make_mlp(dims_t, 0), _lib.make_mlp(dims_o, n[0]), _lib.make_mlp(dims_c, n[0] + n[1])
    a.n_mlp_params, a.color_chn, a.mlp_params = sum(n), color_chn, FAKE + 0x20000
    a.ray_length, a.neg_log_t, a.feature = FAKE + 0x30000, FAKE + 0x31000, FAKE + 0x32000
    a.kernel = _lib.LP_KERNEL_GENERIC
    return a


def _refused(call, a, what, match):
    L = _lib.lib()
    with pytest.raises(_lib.LightplaneHipError, match=match):
        _lib.check(call(L)(ctypes.byref(a), None), what)


RENDERER_CALLS = (("lp_renderer_forward", lambda L: L.lp_renderer_forward), ("lp_renderer_backward", lambda L: L.lp_renderer_backward))
SPLATTER_CALLS = (("lp_splatter_forward", lambda L: L.lp_splatter_forward), ("lp_splatter_backward", lambda L: L.lp_splatter_backward))


def test_layer_widths_summing_past_1024_are_refused():
    """every width is legal, their sum is more than the private activation array holds: LP_EUNSUPPORTED before the launch"""
    wide = [128] * 5
    for what, call in RENDERER_CALLS:
        a = _renderer_args(128, wide, [128, 128, 128, 1], [128, 128, 128, 16])
        _refused(call, a, what, "unsupported shape.*sum of layer widths 1297 exceeds 1024")
    for what, call in SPLATTER_CALLS:
        a = _splatter_args([128] * 9)
        _refused(call, a, what, "unsupported shape.*sum of layer widths 1152 exceeds 1024")


def _splatter_args(dims=None, C=32, n_rays=1):
    a = _lib.LpSplatterArgs()
    a.rays.n_rays = n_rays
    for k, f in enumerate(("directions", "origins", "grid_idx", "near_t", "far_t", "encoding")):
        setattr(a.rays, f, FAKE + 0x1000 * k)
    a.march = _lib.make_march(8, 0, False, False, 1e-5)
    a.out = _lib.make_grid_list(None, [grids.GridDesc(1, 4, 4, 4, 0)], dims[-1] if dims else C, 64)
    a.out.data = FAKE + 0x10000
    a.out_feature, a.out_weight, a.grad_out, a.weight, a.grad_encoding = (FAKE + 0x40000 + 0x1000 * k for k in range(5))
    a.rays.encoding_dim = dims[0] if dims else C
    a.kernel = _lib.LP_KERNEL_GENERIC
    if dims:
        a.input_grid = _lib.make_grid_list(None, [grids.GridDesc(1, 3, 4, 5, 0)], dims[0], 60)
        a.input_grid.data = FAKE + 0x50000
        a.mlp = _lib.make_mlp(dims, 0)
        a.n_mlp_params, a.mlp_params = params.mlp_numel(dims), FAKE + 0x20000
    return a


def test_a_width_of_129_is_refused():
    for what, call in RENDERER_CALLS:
        _refused(call, _renderer_args(16, [16, 129, 32], [32, 32, 1], [32, 32, 16]), what, "unsupported shape.*trunk MLP: width 129 of layer 1")
        _refused(call, _renderer_args(16, [16, 32, 32], [32, 129, 1], [32, 32, 16]), what, "unsupported shape.*opacity MLP: width 129")
        _refused(call, _renderer_args(16, [16, 32, 32], [32, 32, 1], [32, 32, 129], color_chn=129), what, "unsupported shape.*color MLP: width 129")
        _refused(call, _renderer_args(129, [129, 32, 32], [32, 32, 1], [32, 32, 16]), what, "unsupported shape.*129 channels outside")
    for what, call in SPLATTER_CALLS:
        _refused(call, _splatter_args(C=129), what, "unsupported shape.*129")
        _refused(call, _splatter_args([32, 129, 32]), what, "unsupported shape.*width 129")
    e = _lib.LpRayEmbedArgs()
    e.n_rays, e.n_harmonics, e.out_dim = 0, 3, 129
    _refused(lambda L: L.lp_ray_embedding_forward, e, "lp_ray_embedding_forward", "unsupported shape.*out_dim 129")
    e.n_harmonics, e.out_dim = 11, 32
    _refused(lambda L: L.lp_ray_embedding_backward, e, "lp_ray_embedding_backward", "unsupported shape.*n_harmonics 11")


def test_zero_channels_are_refused():
    for what, call in RENDERER_CALLS:
        _refused(call, _renderer_args(0, [0, 32, 32], [32, 32, 1], [32, 32, 16]), what, "unsupported shape.*0 channels outside")
    for what, call in SPLATTER_CALLS:
        _refused(call, _splatter_args(C=0), what, "unsupported shape.*0 channels outside")
    e = _lib.LpRayEmbedArgs()
    e.n_rays, e.n_harmonics, e.out_dim = 0, 3, 0
    _refused(lambda L: L.lp_ray_embedding_forward, e, "lp_ray_embedding_forward", "unsupported shape.*out_dim 0")


def test_the_fused_embedding_stops_at_its_lds_tile():
    """256 * (6 n + 3 + 1 + E + 1) * 4 bytes <= 150 KB (lp_ray_embedding.hip, the backward's staging tile): (10, 85) is the last width
    at ten harmonics, eleven harmonics are beyond the kernel's private embedding array"""
    assert _fused_embedding_supported(10, 85)
    assert 256 * (6 * 10 + 3 + 1 + 85 + 1) * 4 == 150 * 1024
    assert not _fused_embedding_supported(10, 86)
    assert not _fused_embedding_supported(11, 32)
    for n_h, e, _ in R.EMBEDDING_CASES:
        assert _fused_embedding_supported(n_h, e), (n_h, e)

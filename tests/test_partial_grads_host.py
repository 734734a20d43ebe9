"""The table of tests/partial_grad_cases.py without a GPU: every entry lands on the kernel it names (the library's own host
queries), the table reaches every selection the partial-gradient paths differ in, and the subset lists are complete.  A table entry
that silently landed on another kernel would make tests/test_gpu_partial_grads.py test nothing new."""
import itertools

import pytest

import lightplane_amd as lp
from lightplane_amd import _lib
from tests import partial_grad_cases as T

RENDERER_IDS = ["tuned_tri_c16", "tuned_vox_c32", "tuned_nonplain", "tuned_seg", "tuned_nw8", "tuned_tm", "tuned_fp32", "loop_deep_424",
                "loop_shallow_h16", "loop_h64_two_block", "loop_c64", "loop_seg", "loop_two_grid", "loop_two_grid_h64", "generic_lds",
                "generic_global", "flat_grid"]
SPLATTER_IDS = ["mlp_loop_h32", "mlp_loop_two_block", "mlp_loop_seg", "mlp_generic"]


def test_table_holds_the_entries():
    assert [e.id for e in T.RENDERER_ENTRIES] == RENDERER_IDS
    assert [e.id for e in T.SPLATTER_ENTRIES] == SPLATTER_IDS
    for e in T.RENDERER_ENTRIES + T.SPLATTER_ENTRIES:
        assert e.path and e.case.n_rays == T.N_RAYS == 160  # one full four-wave workgroup + a tail with a partial wave
    for e in T.RENDERER_ENTRIES:
        assert all(4 <= n <= 8 for n in e.case.grid_base[1:4])  # the grid sizes of tests/synth.py


@pytest.mark.parametrize("e", T.RENDERER_ENTRIES, ids=lambda e: e.id)
def test_renderer_entry_lands_on_its_kernel(e):
    d = e.case.build()
    before = {k: getattr(lp.config, k) for k in ("segment_forward", "segment_backward", "arithmetic")}
    sel = T.renderer_selection(e, d)
    assert before == {k: getattr(lp.config, k) for k in before}, "renderer_selection left a config attribute changed"
    assert sel["family"] == e.family, sel
    assert sel["segments"] == e.segments, sel
    cfg = d["cfg"]
    S = cfg["num_samples"]
    if e.segmented:
        # 21 samples: three LP_SEG_LEN blocks, the last one partial
        assert e.config == {} and S == 21 and e.segments == -(-S // _lib.LP_SEG_LEN) == 3 and S % _lib.LP_SEG_LEN != 0
    elif sel["offered_segments"] > 1:
        assert e.config.get("segment_backward") is False and e.config.get("segment_forward") is False  # the switch is what keeps it at one sweep
    assert sel["march"] == ("samples" if e.id == "tuned_tm" else "rays")
    if e.id == "tuned_tm":
        assert S == 33 and cfg["num_samples_inf"] == 0
    assert e.two_grid == (d["color_grids"] is not None) == e.id.startswith("loop_two_grid")
    assert (e.arithmetic == _lib.LP_ARITH_FP32) == (e.id == "tuned_fp32")
    if e.id == "tuned_nw8":
        assert cfg["num_samples_inf"] > 64  # eight-wave workgroups
    else:
        assert cfg["num_samples_inf"] <= 64
    if e.id == "tuned_nonplain":
        assert cfg["contract_coords"] and cfg["num_samples_inf"] == 3 and cfg["inject_noise_sigma"] > 0
    if e.id in ("tuned_tri_c16", "tuned_vox_c32"):  # the plain instantiation: nothing that needs per-sample bookkeeping
        assert not cfg["contract_coords"] and cfg["num_samples_inf"] == 0 and cfg["inject_noise_sigma"] == 0 and d["scaffold"] is None
        assert int(d["grids"][0].shape[-1]) == (16 if e.id == "tuned_tri_c16" else 32) and len(d["grids"]) == (3 if e.id == "tuned_tri_c16" else 1)
    if e.flat:
        assert len(d["grids"]) > 1


def test_generic_entries_sit_on_both_sides_of_the_lds_accumulator():
    """lp_renderer_generic.hip: lds_acc = grad_mlp_params && 128 * (widest layer + 1) * 4 + 4 * n_mlp_params <= 96 KB."""
    def lds_bytes(e):
        d = e.case.build()
        dec = d["decoder"]
        widest = max([int(d["grids"][0].shape[-1])] + [int(v) for t in (dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color) for v in t])
        return 128 * (widest + 1) * 4 + 4 * dec.mlp_params.numel(), dec
    small, dec = lds_bytes(T.renderer_entry("generic_lds"))
    assert small <= 96 * 1024
    assert [len(t) - 1 for t in (dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color)] == [2, 2, 2] and int(dec.n_hidden_trunk[1]) == 32
    big, dec = lds_bytes(T.renderer_entry("generic_global"))
    assert 4 * dec.mlp_params.numel() > 96 * 1024 and big > 96 * 1024
    assert sum(int(v) for t in (dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color) for v in t) <= 1024  # what the generic kernels take


@pytest.mark.parametrize("e", T.SPLATTER_ENTRIES, ids=lambda e: e.id)
def test_splatter_entry_lands_on_its_kernel(e):
    sel = T.splatter_selection(e)
    assert sel["family"] == e.family, sel
    assert sel["blocks"] == e.blocks, sel
    assert sel["native_family"] == 3  # a looped shape; mlp_generic forces the shape-generic kernels onto it
    assert sel["segments"] == e.segments, sel
    assert (e.segments > 1) == (e.id == "mlp_loop_seg") == (e.case.num_samples == 70)  # (the sample count of test_mlp_splatter_segmented_march)
    assert (e.kernel == _lib.LP_KERNEL_GENERIC) == (e.id == "mlp_generic")


def test_table_covers_every_selection():
    R = T.RENDERER_ENTRIES
    sels = {e.id: T.renderer_selection(e) for e in R}
    assert {s["family"] for s in sels.values()} == {0, 1, 3}
    for fam in (1, 3):  # both MFMA families, one sweep and segmented
        assert {s["segments"] > 1 for s in sels.values() if s["family"] == fam} == {False, True}
    assert {s["march"] for s in sels.values()} == {"rays", "samples"}
    assert {e.arithmetic for e in R} == {_lib.LP_ARITH_DEFAULT, _lib.LP_ARITH_FP32}
    assert {e.two_grid for e in R} == {False, True}
    assert {e.flat for e in R} == {False, True}
    S = {e.id: T.splatter_selection(e) for e in T.SPLATTER_ENTRIES}
    assert {s["family"] for s in S.values()} == {0, 3}
    assert {s["segments"] > 1 for s in S.values()} == {False, True}
    assert {s["blocks"] for s in S.values()} == {0, 1, 2}


def test_subset_lists_are_complete():
    base = {("P",), ("E",), ("G",), ("P", "E"), ("P", "G"), ("E", "G")}
    two = {("Cg",), ("G", "Cg"), ("P", "Cg")}
    n_single = 0
    for e in T.RENDERER_ENTRIES:
        subs = e.subsets()
        assert len(set(subs)) == len(subs), f"{e.id}: a subset twice"
        want = base | (two if e.two_grid else set())
        extra = set(subs) - want
        assert want <= set(subs), f"{e.id}: misses {want - set(subs)}"
        assert extra <= {("G1",)}, f"{e.id}: {extra}"
        if extra:  # one grid tensor of a list alone: a triplane list entry
            n_single += 1
            assert e.case.is_triplane and not e.flat
        leaves = {"P", "E", "G", "G1"} | ({"Cg"} if e.two_grid else set())
        assert all(set(s) <= leaves and 0 < len(s) for s in subs)
    assert n_single == 1
    # MLP-Splatter: all non-empty proper subsets of {encoding, mlp_params, input grids}
    want = {s for k in (1, 2) for s in itertools.combinations(("E", "P", "G"), k)}
    assert len(want) == 6
    for e in T.SPLATTER_ENTRIES:
        assert set(e.subsets()) == want and len(e.subsets()) == 6


def test_null_upstream_table():
    assert T.NULL_UPSTREAM_ENTRIES == ("tuned_tri_c16", "tuned_seg", "tuned_tm", "tuned_nw8", "loop_deep_424", "loop_two_grid", "generic_lds")
    for i in T.NULL_UPSTREAM_ENTRIES:
        T.renderer_entry(i)
    assert T.NULL_UPSTREAM_PATTERNS == {"len": (True, False, False), "feature": (False, False, True), "nlt": (False, True, False),
                                        "len+feature": (True, False, True)}


def test_gpu_file_collects_every_pair():
    """tests/test_gpu_partial_grads.py is parametrised over exactly the (entry, subset) pairs of the table."""
    from tests import test_gpu_partial_grads as G
    assert G.RENDERER_PAIRS == [(e.id, s) for e in T.RENDERER_ENTRIES for s in e.subsets()]
    assert G.SPLATTER_PAIRS == [(e.id, s) for e in T.SPLATTER_ENTRIES for s in e.subsets()]
    assert len(G.RENDERER_PAIRS) == 17 * 6 + 2 * 3 + 1 and len(G.SPLATTER_PAIRS) == 4 * 6
    assert G.NULL_PAIRS == [(i, p) for i in T.NULL_UPSTREAM_ENTRIES for p in T.NULL_UPSTREAM_PATTERNS]

"""The backward kernels with only SOME gradients requested, and with upstream gradients left out.

include/lightplane_hip.h: a backward's result buffers are "NULL = skip", its upstream gradients "NULL = zeros"; the front-ends pass
NULL for every leaf that does not require a gradient.  The kernels turn those NULLs into other control flow (no workgroup barrier
and no dW tiles in the tuned family's sample loop without ``grad_mlp_params``, no dX product of trunk layer 1 and no scatter
without a grid buffer, another LDS layout of the shape-generic launches, ...): tests/partial_grad_cases.py lists one launch per such
path, this file runs every (launch, subset of leaves) pair of it.

Per launch, once (module-level cache, as ``_REF`` of tests/test_gpu_layouts.py): the BASELINE -- the same call with every leaf
requiring a gradient and all upstream gradients given -- is held to the fp64 oracle with the suite's own machinery and bars
(``forced_oracle_check`` / ``forced_oracle_check_mlp_splatter`` where the kernel has a dump twin, ``assert_grad_close`` with
``TieMasks`` where it has none; 1e-4 of the tensor's largest entry).

Per (launch, subset):
1. the Renderer's outputs are bit-identical to the baseline's (its forward has no atomics; which leaves require a gradient must not
   reach it); the MLP-Splatter's, accumulated with atomics, agree at the bar of 4;
2. leaves outside the subset have ``.grad is None``, leaves inside a gradient of their own shape -- and the pointers that reach the
   C ABI are NULL exactly for the buffers nobody asked for (a spy on the library call), so the partial path really ran;
3. ``grad_encoding`` is bit-identical to the baseline's wherever the header calls it "written" (every one-sweep backward): a plain
   store of arithmetic that depends on neither ``want_params`` nor ``gg``, run-time flags of one binary;
4. every other requested gradient agrees with the baseline's within 2e-5 of the baseline tensor's largest entry -- the project's bar
   for "the same kernel on the same inputs, atomics landing in another order" (tests/test_gpu_layouts.py, ``/baseline``).

The MLP-Splatter's backward reads the forward's splatted WEIGHT grid, which the forward accumulates with atomics: two forwards of
the same call need not leave the same bits there.  3 is a statement about the backward, so a subset run's backward is handed the
baseline forward's weight grid (a saved-tensor hook; no production code is touched): both backwards then see the same inputs.

Upstream gradients left out: autograd materialises zeros for unused outputs, so from Python a NULL upstream pointer never reaches the
kernels; ``LightplaneFunction.backward`` is wrapped (monkeypatch) so that chosen ones of ``g_len`` / ``g_nlt`` / ``g_feat`` arrive
as ``None`` -- which the package's backward already maps to NULL -- and the result is compared with explicit zero tensors."""
import ctypes

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib
from tests import partial_grad_cases as T
from tests.partial_grad_cases import config_set, subset_id
from tests.test_gpu_coherent import oracle_renderer64
from tests.test_gpu_parity import (REL_TOL, TieMasks, _assert_close, _dev, assert_grad_close, forced_oracle_check,
                                   forced_oracle_check_mlp_splatter, has_dump_twin, run_oracle_renderer)

pytestmark = pytest.mark.gpu

BAR = 2e-5   # tests/test_gpu_layouts.py: _assert_close(nm + "/baseline", ..., 2e-5)
ALL = ("P", "E", "G", "Cg")

RENDERER_PAIRS = [(e.id, s) for e in T.RENDERER_ENTRIES for s in e.subsets()]
SPLATTER_PAIRS = [(e.id, s) for e in T.SPLATTER_ENTRIES for s in e.subsets()]
NULL_PAIRS = [(i, p) for i in T.NULL_UPSTREAM_ENTRIES for p in T.NULL_UPSTREAM_PATTERNS]
_BASE = {}   # entry id -> (entry, inputs, baseline results); computed once, never modified

LAST_BACKWARD = {(1, "rays"): b"tuned family, rays per wavefront", (1, "samples"): b"transposed march", (3, "rays"): b"layer-looped family",
                 (0, "rays"): b"shape-generic kernels"}


def _ratio(got, want):
    """max |got - want| / max |want|: the layouts test's figure"""
    scale = max(float(want.abs().max()), 1e-30)
    return float((got.double() - want.double()).abs().max()) / scale


def _close(tag, got, want, worst=None):
    r = _ratio(got, want)
    print(f"partial-grad {tag}: ratio {r:.3e}")
    if worst is not None:
        worst.append(r)
    assert r <= BAR, f"{tag}: differs from the baseline by {r:.3e} of its largest entry (bar {BAR:g})"


def _bit_identical(tag, got, want):
    n = int((got != want).sum())
    print(f"partial-grad {tag}: {n} of {want.numel()} entries differ" + (f" (ratio {_ratio(got, want):.3e})" if n else ""))
    assert got.shape == want.shape and n == 0, f"{tag}: {n} of {want.numel()} entries are not bit-identical to the baseline (ratio {_ratio(got, want):.3e})"


class _Spy:
    """Records the argument block of every call of one library entry point (``lp_renderer_backward``, ``lp_splatter_backward``): which
    pointers reach the C ABI as NULL."""

    def __init__(self, monkeypatch, name, fields, lists=()):
        self.calls = []
        L = _lib.lib()
        orig = getattr(L, name)

        def spy(a_ref, stream):
            a = a_ref._obj
            rec = {f: bool(getattr(a, f)) for f in fields}
            rec.update({f: bool(getattr(a, f)[0]) for f in lists})
            self.calls.append(rec)
            return orig(a_ref, stream)

        monkeypatch.setattr(L, name, spy)


# ---- Renderer ------------------------------------------------------------------------------------------------------------------
def run_renderer(e, d, dev, subset, upstream=None):
    """The entry's call with exactly the leaves of ``subset`` requiring a gradient.  ``upstream``: the three upstream gradients
    (default: the case's own).  Returns dict(out, P, E, G, Cg): detached outputs and the leaves' ``.grad`` (lists for G / Cg)."""
    need = set(subset)
    rays = d["rays"].to(dev)
    rays.encoding = rays.encoding.clone().requires_grad_("E" in need)
    dec = d["decoder"]
    params = dec.mlp_params.to(dev).clone().requires_grad_("P" in need)
    hdec = lp.DecoderParams(params, dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
    kw = {}
    if e.flat:
        flat, sizes = lp.flatten_grid([g.to(dev) for g in d["grids"]])
        grids = [flat.clone().requires_grad_("G" in need)]
        grid_arg, kw = grids[0], dict(grid_sizes=sizes.tolist())
    else:
        grids = [g.to(dev).clone().requires_grad_("G" in need or (i == 1 and "G1" in need)) for i, g in enumerate(d["grids"])]
        grid_arg = grids
    cgrids = None if d["color_grids"] is None else [g.to(dev).clone().requires_grad_("Cg" in need) for g in d["color_grids"]]
    scaffold = None if d["scaffold"] is None else d["scaffold"].to(dev)
    ups = [u.to(dev) for u in (d["upstream"] if upstream is None else upstream)]
    with config_set(**e.config):
        out = lp.lightplane_renderer(rays, grid_arg, hdec, scaffold=scaffold, color_grid=cgrids, **e.call_kwargs(), **d["cfg"], **kw)
        torch.autograd.backward(list(out), ups)
    torch.cuda.synchronize()
    return dict(out=[o.detach() for o in out], P=params.grad, E=rays.encoding.grad, G=[g.grad for g in grids],
                Cg=None if cgrids is None else [g.grad for g in cgrids])


def _last_backward():
    fn = _lib.lib().lp_debug_last_renderer_backward
    fn.restype = ctypes.c_char_p
    return fn()


def _baseline_meets_the_oracle(e, d, dev, base, tag=None):
    """The suite's own oracle machinery, unchanged, on the all-leaves call of the entry; ``base`` (the same call through this file's
    runner) is the very launch it proves: outputs bit-identical, gradients up to the order of the atomics."""
    tag = tag or f"partial-grad baseline {e.id}"
    with config_set(**e.config):
        twin = has_dump_twin(d, kernel=e.kernel, march_order=e.march_order)
        if twin:
            _, prod, _ = forced_oracle_check(tag, d, dev, kernel=e.kernel, march_order=e.march_order, return_results=True)
    if twin:
        out, gp, ge, gg, gc = prod
        for nm, a, b in zip(("ray_length", "neg_log_t", "feature"), base["out"], out):
            if e.flat:  # the proven launch takes the list form of the same grids (tests/test_gpu_parity.py: test_flat_grid_input_and_tail_rays)
                assert torch.allclose(a, b.detach(), rtol=1e-6, atol=1e-6), f"{tag}: {nm}"
            else:
                _bit_identical(f"{tag} {nm} vs the proven launch", a, b.detach())
        _close(f"{tag} grad_mlp_params vs the proven launch", base["P"], gp)
        if e.encoding_is_written and not e.flat:
            _bit_identical(f"{tag} grad_encoding vs the proven launch", base["E"], ge)
        else:
            _close(f"{tag} grad_encoding vs the proven launch", base["E"], ge)
        if e.flat:
            _close(f"{tag} flat grad_grid vs the proven launch", base["G"][0], torch.cat([g.reshape(-1, g.shape[-1]) for g in gg], dim=0))
        else:
            for i, (a, b) in enumerate(zip(base["G"], gg)):
                _close(f"{tag} grad_grid{i} vs the proven launch", a, b)
        for i, (a, b) in enumerate(zip(base["Cg"] or [], gc or [])):
            _close(f"{tag} grad_color_grid{i} vs the proven launch", a, b)
        return
    # no dump twin (eight-wave workgroups, LP_ARITH_FP32): the counted ReLU-flip allowance against the fp32 and fp64 oracles
    assert not e.flat and not e.two_grid
    o_out, o_gp, o_ge, o_gg, _ = run_oracle_renderer(d)
    for nm, a, b in zip(("ray_length", "neg_log_t", "feature"), base["out"], o_out):
        _assert_close(f"{tag}: {nm}", a, b.detach().numpy(), REL_TOL)
    C = d["grids"][0].shape[-1]
    width = max(int(v) for v in list(d["decoder"].n_hidden_trunk) + list(d["decoder"].n_hidden_color))
    q = []

    def oracle64():
        if not q:
            q.append(oracle_renderer64(d))
        return q[0]

    ties = TieMasks(d)
    assert_grad_close(f"{tag}: grad_mlp_params", base["P"], o_gp.numpy(), 4 * width, tol=REL_TOL, want64=lambda: oracle64()[1].numpy(),
                      tie_mask=ties.params_mask())
    assert_grad_close(f"{tag}: grad_encoding", base["E"], o_ge.numpy(), base["E"].shape[1], tol=REL_TOL, want64=lambda: oracle64()[2].numpy(),
                      tie_mask=ties.encoding_mask())
    for i, (a, b) in enumerate(zip(base["G"], o_gg)):
        assert_grad_close(f"{tag}: grad_grid{i}", a, b.numpy(), 8 * C, tol=REL_TOL, want64=lambda i=i: oracle64()[3][i].numpy(),
                          tie_mask=ties.grid_mask(i))


def _renderer_baseline(entry_id):
    if entry_id not in _BASE:
        dev = _dev()
        e = T.renderer_entry(entry_id)
        d = e.case.build()
        sel = T.renderer_selection(e, d)
        assert (sel["family"], sel["segments"]) == (e.family, e.segments), sel
        base = run_renderer(e, d, dev, ALL)
        assert LAST_BACKWARD[(sel["family"], sel["march"])] in _last_backward(), f"{e.id}: the backward that ran is {_last_backward()}"
        _baseline_meets_the_oracle(e, d, dev, base)
        _BASE[entry_id] = (e, d, base)
    return _BASE[entry_id]


def _compare_renderer(tag, e, got, base, subset, worst):
    """Rules 2-4 of the module docstring on one run."""
    need = set(subset)
    for leaf in ("P", "E"):
        g = got[leaf]
        if leaf in need:
            assert g is not None and g.shape == base[leaf].shape, f"{tag}: no gradient on {leaf}"
        else:
            assert g is None, f"{tag}: {leaf} is not in the subset and has a gradient"
    for leaf, key in (("G", "G"), ("Cg", "Cg")):
        for i, g in enumerate(got[key] or []):
            if leaf in need or (leaf == "G" and i == 1 and "G1" in need):
                assert g is not None and g.shape == base[key][i].shape, f"{tag}: no gradient on {key}[{i}]"
                _close(f"{tag} grad_{'grid' if key == 'G' else 'color_grid'}{i}", g, base[key][i], worst)
            else:
                assert g is None, f"{tag}: {key}[{i}] is not in the subset and has a gradient"
    if "P" in need:
        _close(f"{tag} grad_mlp_params", got["P"], base["P"], worst)
    if "E" in need:
        if e.encoding_is_written:
            _bit_identical(f"{tag} grad_encoding", got["E"], base["E"])
        else:
            _close(f"{tag} grad_encoding (accumulated over the segments)", got["E"], base["E"], worst)


@pytest.mark.parametrize("entry_id,subset", RENDERER_PAIRS, ids=[f"{i}-{subset_id(s)}" for i, s in RENDERER_PAIRS])
def test_renderer_partial_gradients(entry_id, subset, monkeypatch):
    dev = _dev()
    e, d, base = _renderer_baseline(entry_id)
    spy = _Spy(monkeypatch, "lp_renderer_backward", ("grad_mlp_params", "grad_encoding", "grad_grid", "grad_color_grid"),
               ("grad_grid_list", "grad_color_grid_list"))
    got = run_renderer(e, d, dev, subset)
    tag = f"{entry_id} [{subset_id(subset)}]"
    # the partial path ran: the buffers nobody asked for reached the library as NULL pointers
    assert len(spy.calls) == 1, f"{tag}: {len(spy.calls)} calls of lp_renderer_backward"
    c = spy.calls[0]
    want_g = "G" in subset or "G1" in subset
    assert c["grad_mlp_params"] == ("P" in subset) and c["grad_encoding"] == ("E" in subset), (tag, c)
    assert (c["grad_grid"], c["grad_grid_list"]) == ((want_g, False) if e.flat else (False, want_g)), (tag, c)
    assert (c["grad_color_grid"], c["grad_color_grid_list"]) == (False, "Cg" in subset), (tag, c)
    for nm, a, b in zip(("ray_length", "neg_log_t", "feature"), got["out"], base["out"]):
        _bit_identical(f"{tag} {nm}", a, b)
    worst = []
    _compare_renderer(tag, e, got, base, subset, worst)
    print(f"partial-grad worst {entry_id} [{subset_id(subset)}]: {max(worst) if worst else 0.0:.3e}")


@pytest.mark.parametrize("entry_id,pattern", NULL_PAIRS, ids=[f"{i}-{p}" for i, p in NULL_PAIRS])
def test_upstream_gradients_left_out(entry_id, pattern, monkeypatch):
    """NULL = zeros: the kernels substitute 0.0f for an upstream gradient that is not given, so the result is that of explicit zero
    tensors -- ``grad_encoding`` bit for bit where it is written, the rest up to the order of the atomics."""
    from lightplane_amd.renderer import LightplaneFunction
    dev = _dev()
    e, d, _ = _renderer_baseline(entry_id)
    given = T.NULL_UPSTREAM_PATTERNS[pattern]
    ups = [u if keep else torch.zeros_like(u) for u, keep in zip(d["upstream"], given)]
    ref = run_renderer(e, d, dev, ALL, upstream=ups)
    assert all(float(g.abs().max()) > 0 for g in [ref["P"]] + ref["G"]), "the comparison is between zeros"  # (the encoding feeds the colour head only)

    spy = _Spy(monkeypatch, "lp_renderer_backward", ("grad_ray_length", "grad_neg_log_t", "grad_feature"))
    wrapped_calls = []
    package_backward = LightplaneFunction.backward

    def backward(ctx, g_len, g_nlt, g_feat, g_alpha):
        gs = [g if keep else None for g, keep in zip((g_len, g_nlt, g_feat), given)]
        wrapped_calls.append([g is not None for g in gs])
        return package_backward(ctx, *gs, g_alpha)

    monkeypatch.setattr(LightplaneFunction, "backward", staticmethod(backward))
    got = run_renderer(e, d, dev, ALL, upstream=ups)
    tag = f"{entry_id} [upstream: {pattern} only]"
    assert wrapped_calls == [list(given)], f"{tag}: the wrapper saw {wrapped_calls}"
    assert len(spy.calls) == 1 and tuple(spy.calls[0][f] for f in ("grad_ray_length", "grad_neg_log_t", "grad_feature")) == given, (tag, spy.calls)
    for nm, a, b in zip(("ray_length", "neg_log_t", "feature"), got["out"], ref["out"]):
        _bit_identical(f"{tag} {nm}", a, b)
    worst = []
    _compare_renderer(tag, e, got, ref, ALL, worst)
    print(f"partial-grad worst {entry_id} [upstream: {pattern}]: {max(worst):.3e}")


# ---- MLP-Splatter ----------------------------------------------------------------------------------------------------------------
class _WeightGrid:
    """Saved-tensor hook of an MLP-Splatter call: keeps the first tensor the forward saves -- the splatted weight grid
    (LightplaneMLPSplatterFunction.forward) -- and, given a replacement, hands the backward that one instead."""

    def __init__(self, replacement=None):
        self.k, self.saved, self.replacement = 0, None, replacement

    def pack(self, t):
        self.k += 1
        if self.k > 1:
            return t
        self.saved = t
        if self.replacement is None:
            return t
        assert t.ndim == 1 and t.shape == self.replacement.shape and t.dtype == self.replacement.dtype
        return self.replacement

    @staticmethod
    def unpack(t):
        return t


def run_mlp_splatter(e, d, dev, subset, weight=None):
    """The entry's call with the leaves of ``subset`` requiring a gradient (E encoding, P mlp_params, G input grids); ``weight``: the
    weight grid the backward reads instead of this forward's.  Returns dict(out, E, P, G, weight)."""
    need = set(subset)
    rays = d["rays"].to(dev)
    rays.encoding = rays.encoding.clone().requires_grad_("E" in need)
    mlp = d["mlp"]
    params = mlp.mlp_params.to(dev).clone().requires_grad_("P" in need)
    hmlp = lp.SplatterParams(params, mlp.n_hidden)
    in_grids = [g.to(dev).clone().requires_grad_("G" in need) for g in d["in_grids"]]
    hook = _WeightGrid(weight)
    with torch.autograd.graph.saved_tensors_hooks(hook.pack, hook.unpack):
        out = lp.lightplane_mlp_splatter(rays, d["out_sizes"], hmlp, in_grids, kernel=e.kernel, **d["cfg"])
    assert hook.k >= 8 + len(in_grids) and hook.saved.shape == (sum(o.numel() // o.shape[-1] for o in out),)
    torch.autograd.backward(out, [u.to(dev) for u in d["upstream"]])
    torch.cuda.synchronize()
    return dict(out=[o.detach() for o in out], E=rays.encoding.grad, P=params.grad, G=[g.grad for g in in_grids], weight=hook.saved.detach())


def _splatter_baseline(entry_id):
    if entry_id not in _BASE:
        dev = _dev()
        e = next(x for x in T.SPLATTER_ENTRIES if x.id == entry_id)
        d = e.case.build()
        sel = T.splatter_selection(e, d)
        assert sel["family"] == e.family and (sel["segments"] > 1) == (not e.encoding_is_written), sel
        base = run_mlp_splatter(e, d, dev, ("E", "P", "G"))
        tag = f"partial-grad baseline {e.id}"
        _, (out, ge, gp, gin) = forced_oracle_check_mlp_splatter(tag, d, dev, kernel=e.kernel)
        # the launch the oracle check proved is this call: same kernels on the same inputs, the atomics in another order
        for k, (a, b) in enumerate(zip(base["out"], out)):
            _close(f"{tag} out{k} vs the proven launch", a, b.detach())
        _close(f"{tag} grad_encoding vs the proven launch", base["E"], ge)
        _close(f"{tag} grad_mlp_params vs the proven launch", base["P"], gp)
        for k, (a, b) in enumerate(zip(base["G"], gin)):
            _close(f"{tag} grad_input_grid{k} vs the proven launch", a, b)
        _BASE[entry_id] = (e, d, base)
    return _BASE[entry_id]


@pytest.mark.parametrize("entry_id,subset", SPLATTER_PAIRS, ids=[f"{i}-{subset_id(s)}" for i, s in SPLATTER_PAIRS])
def test_mlp_splatter_partial_gradients(entry_id, subset, monkeypatch):
    dev = _dev()
    e, d, base = _splatter_baseline(entry_id)
    spy = _Spy(monkeypatch, "lp_splatter_backward", ("grad_encoding", "grad_mlp_params", "grad_input_grid"), ("grad_input_grid_list",))
    got = run_mlp_splatter(e, d, dev, subset, weight=base["weight"])
    tag = f"{entry_id} [{subset_id(subset)}]"
    assert len(spy.calls) == 1, f"{tag}: {len(spy.calls)} calls of lp_splatter_backward"
    c = spy.calls[0]
    assert (c["grad_encoding"], c["grad_mlp_params"], c["grad_input_grid"], c["grad_input_grid_list"]) == \
        ("E" in subset, "P" in subset, False, "G" in subset), (tag, c)
    worst = []
    for k, (a, b) in enumerate(zip(got["out"], base["out"])):
        _close(f"{tag} out{k}", a, b, worst)
    _close(f"{tag} weight grid of this forward vs the baseline's", got["weight"], base["weight"], worst)
    for leaf in ("E", "P"):
        g = got[leaf]
        if leaf in subset:
            assert g is not None and g.shape == base[leaf].shape, f"{tag}: no gradient on {leaf}"
        else:
            assert g is None, f"{tag}: {leaf} is not in the subset and has a gradient"
    for k, g in enumerate(got["G"]):
        if "G" in subset:
            assert g is not None and g.shape == base["G"][k].shape, f"{tag}: no gradient on input grid {k}"
            _close(f"{tag} grad_input_grid{k}", g, base["G"][k], worst)
        else:
            assert g is None, f"{tag}: input grid {k} is not in the subset and has a gradient"
    if "P" in subset:
        _close(f"{tag} grad_mlp_params", got["P"], base["P"], worst)
    if "E" in subset:
        if e.encoding_is_written:
            _bit_identical(f"{tag} grad_encoding", got["E"], base["E"])
        else:
            _close(f"{tag} grad_encoding (accumulated over the segments)", got["E"], base["E"], worst)
    print(f"partial-grad worst {entry_id} [{subset_id(subset)}]: {max(worst):.3e}")

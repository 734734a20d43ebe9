"""Every buffer the front-ends allocate uninitialised, poisoned and fenced (tests/guarded_alloc.py), through every kernel file.

Each case runs ONCE unguarded -- the baseline -- and once per poison pattern inside ``guarded(pattern)``, forward and backward, and then
1. every fence is intact: those around the ``torch.zeros`` buffers too (gradient scatters, splat targets);
2. every poisoned buffer (``torch.empty`` / ``empty_like`` in lightplane_amd/) has no element left that still holds the poison, under
   every pattern -- except the elements ``EXEMPT`` names, each with the line of include/lightplane_hip.h that says nobody reads them
   (a byte buffer of packed data, the weight-image workspace, is judged over the pattern set: a written byte equals the byte poison once
   in 256, an unwritten one equals it under both byte poisons);
3. the results are the baseline's: bit for bit where no atomics are involved (the Renderer's outputs, ``grad_encoding`` of a one-sweep
   backward -- bar (a) of tests/test_gpu_partial_grads.py -- and everything else a kernel WRITES from inputs that are themselves
   reproducible), within that file's ``BAR`` = 2e-5 of the baseline tensor's largest entry where atomics accumulate.
Baselines come from case tables the suite already holds to the fp64 oracle; a case that is new here is held to it first, at the
project's 1e-4, with the suite's own helpers.

Who writes and who reads each poisoned buffer (read before the first run; every one holds floats or occupancy bytes -- the one number
that is an index, the last marched sample in the closing checkpoint pair, is written by every forward for every ray and clamped to
``[0, S - 1]`` by every backward before use):

    front-end        buffer            written by                                               read by
    renderer.py      ray_length, nlt,  write_ray_outputs: renderer_fwd_bf3 / _tm / _fwd_combine  the caller; nlt also by every backward
                     feature, alpha      (lp_renderer_mfma.hip), renderer_loop_fwd (lp_renderer_
                                         loop.h, _stream.hip), renderer_fwd (lp_renderer_generic.hip)
                     ckpt              the same forwards, per block of LP_NLT_CKPT samples +      renderer_bwd_* of the same family
                                         the closing pair; the combine pass of a segmented forward  (lp_renderer_mfma_bwd.h:210, :419;
                                                                                                   lp_renderer_loop.h; _generic.hip)
                     seg               the forwards, per block of LP_SEG_LEN samples; rewritten   the segmented backwards
                                         to absolute sums by renderer_fwd_combine
                     ws                the weight-image packing pass of lp_renderer_forward_ws    the streamed forward (LDS ring)
    points.py        opacity, color    points_fwd (lp_points.hip)                                the caller
                     d_points          points_bwd                                                the caller
    point_grid.py    out               point_gather (lp_point_grid.hip)                          the caller
                     d_points          point_grad_points                                         the caller
                     d_features        point_gather of the upstream grids                        the caller
    resample.py      outs, grads       grid_resample_fwd / _bwd (lp_grid_resample.hip)           the caller
    regularizers.py  workspace         grid_tv sweep: one fp64 partial per workgroup             the final reduction of the same call
                     loss              that reduction                                            the caller
                     grads             grid_tv_backward (gather form)                            the caller
    scaffold.py      the result        scaffold_lattice; the dilation's second byte pass         the caller
                     workspace         the dilation's byte passes                                the next byte pass
    ray_clip.py      near, far, hit    rays_clip (lp_ray_clip.hip)                               the caller
    modules.py       out               ray_embedding_fwd (lp_ray_embedding.hip)                  the caller

Measured on an MI355X: DESIGN.md 2, "Unwritten and overrun buffers"."""
import copy
import dataclasses
import math
import os

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib
from oracle import lightplane_oracle as O
from tests import partial_grad_cases as T
from tests import point_grid_cases as PG
from tests import points_cases as PC
from tests import ray_clip_cases as RC
from tests import test_gpu_grid_resample as RS
from tests import test_gpu_grid_tv as TV
from tests import test_gpu_partial_grads as P
from tests import test_gpu_scaffold as SC
from tests.guarded_alloc import _BITS_VIEW, PATTERNS, guarded
from tests.partial_grad_cases import NO_SEG, config_set
from tests.synth import RendererCase
from tests.test_gpu_parity import REL_TOL, TieMasks, _assert_close, _dev, assert_grad_close

pytestmark = pytest.mark.gpu

BAR = P.BAR
ALL = P.ALL
PKG = os.sep + "lightplane_amd" + os.sep

#: (front-end file, buffer) -> why elements of it may stay poisoned, and which (``_may_stay``).  Nothing else may.
EXEMPT = {
    ("renderer.py", "ckpt"): "with stop_transmittance only, and only the pairs behind a ray's last marched sample: include/lightplane_hip.h, "
                             "the comment of LP_NLT_CKPT -- 'with early termination the pairs of checkpoints BEHIND the last marched sample "
                             "are not written, and the backward never reads them'",
    ("renderer.py", "ws"): "the 8 x 16 bytes of row skew in every 2176-byte limb of a block image: include/lightplane_hip.h, "
                           "lp_renderer_forward_workspace_bytes -- 'the packing pass does not write them, and nothing that is computed reads them'",
    ("regularizers.py", "workspace"): "the tail behind the partials of the workgroups that ran: include/lightplane_hip.h, lp_grid_tv_forward -- 'the "
                                      "call writes one partial per workgroup it launches, from the start of the buffer, and reads back exactly "
                                      "those; ... the tail of the buffer is neither written nor read'",
}
LIMB_BYTES, ROW_BYTES = 2176, 64   # a limb of a block image: 32 rows of 64 bytes, row k at 64 k + 16 (k >> 2) (rm_off, csrc/lp_bf3.h)


def _may_stay(r):
    """the elements of record ``r`` that EXEMPT lets keep the poison, as a bool mask over the flat payload; None: none"""
    key = (os.path.basename(r.site[0]), r.name)
    n = r.payload.numel()
    idx = torch.arange(n, device=r.payload.device)
    if key == ("renderer.py", "ws"):
        assert n % LIMB_BYTES == 0
        off = idx % LIMB_BYTES
        covered = torch.zeros(n, dtype=torch.bool, device=idx.device)
        for k in range(32):
            start = ROW_BYTES * k + 16 * (k >> 2)
            covered |= (off >= start) & (off < start + ROW_BYTES)
        return ~covered
    if key == ("regularizers.py", "workspace"):
        mask = r.payload.detach().view(-1).view(torch.int64) == _poison(r)
        first = int(mask.float().argmax())
        assert first >= 1 and bool(mask[first:].all()), f"the unwritten elements are not the tail of the workspace: {r.where()}"
        return idx >= first
    return None


def _poison(r):
    from tests.guarded_alloc import poison_bits
    return poison_bits(r.pattern, r.dtype)


STATS = dict(cases=0, guarded_runs=0, buffers=0, elements=0, fenced=0, exempt_elements=0, worst=0.0, worst_tag="")


def _leaves(x, prefix=""):
    """(name, tensor) over a result: a tensor, None, or dicts / lists / tuples of results"""
    if x is None:
        return
    if torch.is_tensor(x):
        yield prefix, x
    elif isinstance(x, dict):
        for k, v in x.items():
            yield from _leaves(v, f"{prefix}.{k}" if prefix else str(k))
    else:
        for i, v in enumerate(x):
            yield from _leaves(v, f"{prefix}[{i}]")


def _differing_bits(a, b):
    a, b = a.detach().contiguous(), b.detach().contiguous()
    if a.dtype in _BITS_VIEW:
        a, b = a.view(_BITS_VIEW[a.dtype]), b.view(_BITS_VIEW[b.dtype])
    return int((a != b).sum())


def _compare(tag, got, base, bit):
    got, base = dict(_leaves(got)), dict(_leaves(base))
    assert got.keys() == base.keys(), (tag, sorted(got), sorted(base))
    for name, want in base.items():
        g = got[name]
        assert g.shape == want.shape and g.dtype == want.dtype, f"{tag} {name}: {tuple(g.shape)} {g.dtype} vs {tuple(want.shape)} {want.dtype}"
        if any(name == b or name.startswith(b + "[") or name.startswith(b + ".") for b in bit):
            n = _differing_bits(g, want)
            assert n == 0, f"{tag} {name}: {n} of {want.numel()} entries are not bit-identical to the unguarded baseline"
        else:
            assert bool(torch.isfinite(g).all()), f"{tag} {name}: not finite"
            r = P._ratio(g, want)
            if r > STATS["worst"]:
                STATS["worst"], STATS["worst_tag"] = r, f"{tag} {name}"
            assert r <= BAR, f"{tag} {name}: differs from the unguarded baseline by {r:.3e} of its largest entry (bar {BAR:g})"


def library_buffers(g):
    """the poisoned records of a guard whose call site is in the package"""
    return [r for r in g.records if r.poisoned and PKG in r.site[0]]


def check_guarded(tag, run, bit, may_stay=None, expect=None):
    """The rule of the module docstring on one case.  ``run()`` -> result (tensors in dicts / lists); ``bit``: the result names held
    bit for bit; ``may_stay(record)`` -> bool mask over the flat payload of the elements EXEMPT allows to stay poisoned (or None);
    ``expect``: names of poisoned buffers the case has to allocate.  Returns (baseline, the guards)."""
    base = run()
    torch.cuda.synchronize()
    guards, stray_bytes = [], {}
    for p in PATTERNS:
        with guarded(p) as g:
            got = run()
            torch.cuda.synchronize()
        # (leaving the block checked every fence: g.check())
        recs = library_buffers(g)
        names = {r.name for r in recs}
        assert not expect or set(expect) <= names, f"{tag} [{p}]: expected poisoned buffers {sorted(expect)}, the ledger has {sorted(names)}"
        for k, r in enumerate(recs):
            mask = g.unwritten_mask(r)
            n = int(mask.sum())
            allowed = None
            if n:
                allowed = may_stay(r) if may_stay is not None else None
                allowed = _may_stay(r) if allowed is None else allowed
            if allowed is not None:
                key = (os.path.basename(r.site[0]), r.name)
                assert key in EXEMPT, f"{tag}: {key} is not in EXEMPT"
                STATS["exempt_elements"] += int((mask & allowed.to(mask.device)).sum())
                mask = mask & ~allowed.to(mask.device)
                n = int(mask.sum())
            if r.dtype == torch.uint8 and n:
                # a byte of packed data equals the byte poison once in 256: what counts is a byte that holds the poison under BOTH byte
                # poisons of the pattern set (an unwritten byte does; a written one cannot)
                stray_bytes.setdefault(k, []).append((r, mask))
                n = 0
            assert n == 0, (f"{tag} [{p}]: {n} of {mask.numel()} elements were never written (first at flat index "
                            f"{int(mask.nonzero()[0]) if n else -1}): {r.where()}")
            STATS["buffers"] += 1
            STATS["elements"] += mask.numel()
        STATS["fenced"] += sum(1 for r in g.records if r.fences is not None)
        STATS["guarded_runs"] += 1
        _compare(f"{tag} [{p}]", got, base, bit)
        guards.append(g)
    for k, found in stray_bytes.items():
        byte_poisons = {_poison(r) for r, _ in found}
        if len(found) == len(PATTERNS) and len(byte_poisons) > 1:
            both = found[0][1].clone()
            for _, m in found[1:]:
                both &= m
            assert int(both.sum()) == 0, (f"{tag}: {int(both.sum())} bytes hold the poison under every pattern (first at flat index "
                                          f"{int(both.nonzero()[0])}): {found[0][0].where()}")
    STATS["cases"] += 1
    print(f"unwritten-buffers {tag}: {len(PATTERNS)} patterns, {len(library_buffers(guards[0]))} poisoned library buffers "
          f"({sorted({r.name for r in library_buffers(guards[0])})}), {sum(1 for r in guards[0].records if r.fences is not None)} fenced allocations; "
          f"worst ratio so far {STATS['worst']:.3e}")
    return base, guards


# ---- Renderer: the 17 paths of tests/partial_grad_cases.py ---------------------------------------------------------------------
def _renderer_bits(e):
    return ("out", "E") if e.encoding_is_written else ("out",)


def _renderer_expect(e):
    return ("ray_length", "nlt", "feature", "ckpt") + (("seg",) if e.segmented else ())


@pytest.mark.parametrize("entry_id", [e.id for e in T.RENDERER_ENTRIES])
def test_renderer_paths(entry_id):
    dev = _dev()
    e, d, base = P._renderer_baseline(entry_id)   # held to the fp64 oracle there (cached; shared with that file)
    got, _ = check_guarded(f"renderer {entry_id}", lambda: P.run_renderer(e, d, dev, ALL), _renderer_bits(e), expect=_renderer_expect(e))
    # this file's unguarded run is that baseline's launch again
    _compare(f"renderer {entry_id} vs the proven baseline", got, base, _renderer_bits(e))


# ---- ... and the conditions those entries lack, each on one tuned, one looped and one shape-generic entry -------------------------
CARRIERS = ("tuned_tri_c16", "loop_deep_424", "generic_lds")


def _half_empty_scaffold_and_missing_rays(d):
    """a scaffold whose far half (x > 0) is empty, and every fifth ray aimed past the box: origin 3 units out, direction perpendicular
    to it, so that no sample comes closer than 3 to the centre"""
    B = d["grids"][0].shape[0]
    sc = torch.ones(B, 4, 5, 6)
    sc[..., 3:] = 0.0
    d["scaffold"] = sc
    rays = d["rays"]
    gen = torch.Generator().manual_seed(7)
    idx = torch.arange(0, rays.n_rays, 5)
    o = torch.nn.functional.normalize(torch.randn(len(idx), 3, generator=gen), dim=-1) * 3.0
    t = torch.nn.functional.normalize(torch.randn(len(idx), 3, generator=gen), dim=-1)
    rays.origins[idx] = o
    rays.directions[idx] = torch.nn.functional.normalize(torch.cross(o, t, dim=-1), dim=-1)
    rays.near[idx], rays.far[idx] = 0.0, 4.0
    return d


CONDITIONS = {
    "s33": (dict(num_samples=33), None),
    "s40": (dict(num_samples=40), None),
    "inf3": (dict(num_samples_inf=3), None),
    "miss_mask_scaffold": (dict(mask_oob=True), _half_empty_scaffold_and_missing_rays),
}
_NEW = {}


def _new_entry(carrier, cond):
    key = (carrier, cond)
    if key not in _NEW:
        kw, edit = CONDITIONS[cond]
        e0 = T.renderer_entry(carrier)
        e = dataclasses.replace(e0, id=f"{carrier}+{cond}", case=dataclasses.replace(e0.case, **kw))
        d = e.case.build()
        if edit is not None:
            d = edit(d)
        sel = T.renderer_selection(e, d)
        assert (sel["family"], sel["segments"]) == (e.family, 1), sel
        _NEW[key] = (e, d)
    return _NEW[key]


@pytest.mark.parametrize("cond", list(CONDITIONS))
@pytest.mark.parametrize("carrier", CARRIERS)
def test_renderer_conditions(carrier, cond):
    dev = _dev()
    e, d = _new_entry(carrier, cond)
    base, guards = check_guarded(f"renderer {e.id}", lambda: P.run_renderer(e, d, dev, ALL), _renderer_bits(e), expect=_renderer_expect(e))
    if cond == "miss_mask_scaffold":
        miss = torch.arange(0, d["rays"].n_rays, 5)
        assert float(base["out"][1][miss].abs().max()) == 0.0 and float(base["out"][2][miss].abs().max()) == 0.0, "the aimed rays do not miss"
    P._baseline_meets_the_oracle(e, d, dev, base)   # new here: the 1e-4 bar, the suite's own machinery


# ---- early termination -----------------------------------------------------------------------------------------------------------
STOP = 1e-2
STOP_S = 40   # two checkpoint blocks: a wave that stops inside the first never writes the second


class _Saved:
    """saved-tensor hook: keeps what LightplaneFunction.forward saves, in order (nlt, ckpt, ...)"""

    def __init__(self):
        self.t = []

    def pack(self, t):
        self.t.append(t)
        return t

    @staticmethod
    def unpack(t):
        return t


def _oracle(d, dtype, live=None, bg=None, alpha_mode=0, g_alpha=None):
    """The oracle's march (oracle.lightplane_renderer_naive, restated with two hooks) in ``dtype``: ``live [N, S]`` multiplies the
    opacities -- 0 behind the sample at which the kernel's wavefront stopped -- and ``bg`` / ``alpha_mode`` add the module epilogue
    (feature + T * bg; alpha = 1 - T or log T).  Returns (outputs, grad_mlp_params, grad_encoding, grad_grids)."""
    cfg = d["cfg"]
    assert not cfg.get("inject_noise_sigma") and d["color_grids"] is None
    rays = d["rays"]
    near, far, dirs, orig = (getattr(rays, f).to(dtype) for f in ("near", "far", "directions", "origins"))
    enc = rays.encoding.to(dtype).clone().requires_grad_(True)
    dec = copy.copy(d["decoder"])
    dec.mlp_params = dec.mlp_params.to(dtype).clone().requires_grad_(True)
    grids = [g.to(dtype).clone().requires_grad_(True) for g in d["grids"]]
    scaffold = None if d["scaffold"] is None else d["scaffold"].to(dtype)
    S, S_inf = cfg["num_samples"], cfg["num_samples_inf"]
    depths = O.ray_depths(near, far, S, S_inf, 1e-5)
    points = depths[..., None] * dirs[:, None] + orig[:, None]
    delta = O.ray_deltas(near, far, depths, S)
    opacity, color = O.eval_decoder(points, grids, rays.grid_idx, dec, enc, cfg["gain"], mask_out_of_bounds_samples=cfg["mask_out_of_bounds_samples"],
                                    scaffold=scaffold, contract_coords=cfg["contract_coords"])
    if live is not None:
        opacity = opacity * live.to(dtype)
    nlt = torch.cumsum(torch.nn.functional.pad(opacity * delta, (1, 0)), dim=-1)
    tr = torch.exp(-nlt)
    w = tr[:, :-1] - tr[:, 1:]
    out = [(depths * w).sum(-1), nlt[:, -1], (color * w[..., None]).sum(-2)[..., : dec.color_chn]]
    if bg is not None:
        out[2] = out[2] + tr[:, -1, None] * bg.to(dtype)
    ups = [u.to(dtype) for u in d["upstream"]]
    if alpha_mode:
        out.append(1.0 - tr[:, -1] if alpha_mode == 1 else -nlt[:, -1])
        ups.append(g_alpha.to(dtype))
    sum((o * u).sum() for o, u in zip(out, ups)).backward()
    return [o.detach() for o in out], dec.mlp_params.grad, enc.grad, [g.grad for g in grids], nlt.detach()


def _baseline_meets(tag, d, base, names, **okw):
    """outputs at the 1e-4 bar, gradients through assert_grad_close with the fp64 twin and TieMasks: the flip allowance as it is defined
    there (every use shows in the terminal summary)"""
    o32 = _oracle(d, torch.float32, **okw)
    q = []

    def o64():
        if not q:
            q.append(_oracle(d, torch.float64, **okw))
        return q[0]

    for nm, a, b in zip(names, base["out"], o64()[0]):
        _assert_close(f"{tag}: {nm}", a, b.numpy(), REL_TOL)
    C = d["grids"][0].shape[-1]
    width = max(int(v) for v in list(d["decoder"].n_hidden_trunk) + list(d["decoder"].n_hidden_color))
    ties = TieMasks(d)
    assert_grad_close(f"{tag}: grad_mlp_params", base["P"], o32[1].numpy(), 4 * width, tol=REL_TOL, want64=lambda: o64()[1].numpy(), tie_mask=ties.params_mask())
    assert_grad_close(f"{tag}: grad_encoding", base["E"], o32[2].numpy(), base["E"].shape[1], tol=REL_TOL, want64=lambda: o64()[2].numpy(),
                      tie_mask=ties.encoding_mask())
    for i, (a, b) in enumerate(zip(base["G"], o32[3])):
        assert_grad_close(f"{tag}: grad_grid{i}", a, b.numpy(), 8 * C, tol=REL_TOL, want64=lambda i=i: o64()[3][i].numpy(), tie_mask=ties.grid_mask(i))


def _stop_case(carrier):
    """A dense scene (gain x 40) behind a scaffold whose x > 0 half is empty, the rays ordered by how fast they saturate in the exact
    fp64 march: the first wavefronts hold rays that are all opaque within a few samples and stop inside the first checkpoint block, the
    last ones hold rays through the empty half and never stop."""
    key = (carrier, "stop")
    if key not in _NEW:
        e0 = T.renderer_entry(carrier)
        e = dataclasses.replace(e0, id=f"{carrier}+stop", case=dataclasses.replace(e0.case, num_samples=STOP_S, gain=40.0 * e0.case.gain))
        d = e.case.build()
        B = d["grids"][0].shape[0]
        d["scaffold"] = torch.ones(B, 4, 4, 4)
        d["scaffold"][..., :2] = 0.0
        nlt = _oracle_nlt(d)
        limit = -math.log(STOP)
        first = torch.where((nlt[:, 1:] >= limit).any(1), (nlt[:, 1:] >= limit).float().argmax(1), torch.full((nlt.shape[0],), 10 ** 6))
        order = torch.argsort(first, stable=True)
        d["rays"] = d["rays"][order]
        d["upstream"] = tuple(u[order] for u in d["upstream"])
        d["cfg"] = dict(d["cfg"], stop_transmittance=STOP)
        _NEW[key] = (e, d)
    return _NEW[key]


def _oracle_nlt(d):
    """running -log T [N, S + 1] of the exact fp64 march"""
    return _oracle(d, torch.float64)[4]


def _run_saving(e, d, dev):
    hook = _Saved()
    with torch.autograd.graph.saved_tensors_hooks(hook.pack, hook.unpack):
        res = P.run_renderer(e, d, dev, ALL)
    res["s_last"] = hook.t[1].detach().view(d["rays"].n_rays, -1, 2)[:, -1, 0].clone()   # the closing pair: the last marched sample
    return res


@pytest.mark.parametrize("carrier", CARRIERS)
def test_renderer_early_termination(carrier):
    dev = _dev()
    e, d = _stop_case(carrier)
    S, n = STOP_S, d["rays"].n_rays
    n_pairs = _lib.n_nlt_ckpt(S, 0) // 2
    limit = -math.log(STOP)
    state = {}

    def may_stay(r):
        if r.name != "ckpt":
            return None
        # pairs behind the last marched sample (the closing pair holds it), the closing pair itself excluded
        pairs = r.payload.detach().view(n, n_pairs, 2)
        s_last = pairs[:, -1, 0].round().long()
        written = torch.where(s_last >= S - 1, torch.full_like(s_last, n_pairs - 1), (s_last + 1) // _lib.LP_NLT_CKPT)
        k = torch.arange(n_pairs, device=pairs.device)[None]
        allowed = (k >= written[:, None]) & (k < n_pairs - 1)
        state["exempt_pairs"] = int(allowed.sum())
        return allowed[..., None].expand(n, n_pairs, 2).reshape(-1)

    base, guards = check_guarded(f"renderer {e.id}", lambda: _run_saving(e, d, dev), _renderer_bits(e) + ("s_last",), may_stay=may_stay,
                                 expect=_renderer_expect(e))
    assert state.get("exempt_pairs", 0) > 0, "no wavefront stopped inside the first checkpoint block: the exemption is not exercised"
    # where the kernel stopped, checked against the exact fp64 march: every ray of a stopped wavefront is opaque at its last sample, and
    # in every run of rays with one last sample some ray was not yet opaque one sample earlier
    s_last = base["s_last"].round().long().cpu()
    nlt64 = _oracle_nlt(d)
    stopped = s_last < S - 1
    assert int(stopped.sum()) >= 32 and int((~stopped).sum()) >= 32, f"{int(stopped.sum())} of {n} rays stopped: some waves have to, others not"
    assert int(s_last[stopped].min()) < _lib.LP_NLT_CKPT - 1
    at = nlt64.gather(1, (s_last + 1)[:, None])[:, 0]
    assert bool((at[stopped] >= limit * (1 - 1e-4)).all()), "a ray of a stopped wavefront is not opaque in the fp64 march"
    before = nlt64.gather(1, s_last[:, None])[:, 0]
    edges = [0] + (torch.nonzero(s_last[1:] != s_last[:-1]).flatten() + 1).tolist() + [n]
    for lo, hi in zip(edges[:-1], edges[1:]):
        if s_last[lo] > 0 and s_last[lo] < S - 1:
            assert float(before[lo:hi].min()) < limit * (1 + 1e-4), f"rays {lo}..{hi}: opaque one sample before the stop"
    live = (torch.arange(S)[None] <= s_last[:, None])
    base["out"] = base["out"][:3]
    _baseline_meets(f"unwritten-buffers baseline {e.id}", d, base, ("ray_length", "neg_log_t", "feature"), live=live)


# ---- the module epilogue -----------------------------------------------------------------------------------------------------------
def _run_epilogue(e, d, dev, bg, alpha_mode, g_alpha):
    from lightplane_amd.renderer import _render
    rays = d["rays"].to(dev)
    rays.encoding = rays.encoding.clone().requires_grad_(True)
    dec = d["decoder"]
    params = dec.mlp_params.to(dev).clone().requires_grad_(True)
    hdec = lp.DecoderParams(params, dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
    grids = [g.to(dev).clone().requires_grad_(True) for g in d["grids"]]
    with config_set(**e.config):
        out = _render(rays, grids, hdec, bg_color=bg.to(dev), alpha_mode=alpha_mode, **e.call_kwargs(), **d["cfg"])
        torch.autograd.backward(list(out), [u.to(dev) for u in d["upstream"]] + [g_alpha.to(dev)])
    torch.cuda.synchronize()
    return dict(out=[o.detach() for o in out], P=params.grad, E=rays.encoding.grad, G=[g.grad for g in grids])


@pytest.mark.parametrize("alpha_mode", [1, 2])
@pytest.mark.parametrize("carrier", CARRIERS)
def test_renderer_module_epilogue(carrier, alpha_mode):
    dev = _dev()
    e = T.renderer_entry(carrier)
    _, d, _ = P._renderer_baseline(carrier)
    gen = torch.Generator().manual_seed(11 + alpha_mode)
    bg = torch.rand(d["decoder"].color_chn, generator=gen)
    g_alpha = torch.randn(d["rays"].n_rays, generator=gen)
    tag = f"renderer {carrier}+bg+alpha{alpha_mode}"
    base, _ = check_guarded(tag, lambda: _run_epilogue(e, d, dev, bg, alpha_mode, g_alpha), ("out", "E"),
                            expect=("ray_length", "nlt", "feature", "alpha", "ckpt"))
    _baseline_meets(f"unwritten-buffers baseline {tag}", d, base, ("ray_length", "neg_log_t", "feature", "alpha"), bg=bg, alpha_mode=alpha_mode,
                    g_alpha=g_alpha)


# ---- the layer-looped forward of deep hidden-64 decoders (config.deep_forward_mfma) -----------------------------------------------
DEEP = {"resident_322": ((3, 2, 2), 3, ()), "streamed_444": ((4, 4, 4), 4, ("ws",))}


@pytest.mark.parametrize("name", list(DEEP))
def test_renderer_deep_forward(name):
    """the shapes of tests/test_gpu_deep_forward.py::test_shapes_against_oracle (C = 32, voxel grid): resident and streamed weight images"""
    dev = _dev()
    layers, family, extra = DEEP[name]
    case = RendererCase("deep", seed=100 + 32 + sum(layers), n_rays=300, grid_base=(2, 6, 7, 5, 32), is_triplane=False, n_layers=layers, hidden=64,
                        num_samples=21)
    e = T.RendererEntry(f"deep_{name}", "layer-looped forward of a deep hidden-64 decoder, shape-generic backward", case,
                        config=dict(NO_SEG, deep_forward_mfma=True, warn_generic_kernel=False), family=0)
    d = case.build()
    with config_set(**e.config):
        assert lp.forward_kernel_family(d["rays"], d["grids"], d["decoder"]) == family
    base, _ = check_guarded(f"renderer {e.id}", lambda: P.run_renderer(e, d, dev, ALL), _renderer_bits(e), expect=_renderer_expect(e) + extra)
    P._baseline_meets_the_oracle(e, d, dev, base)


# ---- MLP-Splatter -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry_id", [e.id for e in T.SPLATTER_ENTRIES])
def test_mlp_splatter_paths(entry_id):
    """every buffer is an accumulation target (torch.zeros): the fences do the work"""
    dev = _dev()
    e, d, base = P._splatter_baseline(entry_id)
    # (the backward reads the forward's splatted weight grid, accumulated with atomics: every run's backward is handed the baseline's)
    got, guards = check_guarded(f"mlp-splatter {entry_id}", lambda: P.run_mlp_splatter(e, d, dev, ("E", "P", "G"), weight=base["weight"]),
                                ("E",) if e.encoding_is_written else ())
    assert all(sum(1 for r in g.from_file("lightplane_amd/splatter.py") if r.fences is not None) >= 5 for g in guards)
    _compare(f"mlp-splatter {entry_id} vs the proven baseline", got, base, ("E",) if e.encoding_is_written else ())


# ---- decoder at points ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PC.CASES))
def test_decoder_at_points(name):
    dev, c = _dev(), PC.case(name)
    from tests.test_gpu_points import _joint, _opacity_only

    def run():
        d = PC.on_device(c, dev, requires_grad=("points", "params", "enc", "grids", "cgrids"))
        op, col = _joint(d, c)
        ((op * c["u_op"].to(dev)).sum() + (col * c["u_col"].to(dev)).sum()).backward()
        as_list = lambda g: None if g is None else (g if isinstance(g, list) else [g])  # noqa: E731
        res = dict(op=op.detach(), col=col.detach(), d_points=d["pts"].grad, d_params=d["params"].grad, d_enc=d["enc"].grad,
                   d_grids=[t.grad for t in as_list(d["grid"])], d_cgrids=None if d["color_grid"] is None else [t.grad for t in as_list(d["color_grid"])])
        d = PC.on_device(c, dev, requires_grad=("points", "params", "grids"))
        op1 = _opacity_only(d, c)
        (op1 * c["u_op"].to(dev)).sum().backward()
        res.update(op_only=op1.detach(), op_only_d_points=d["pts"].grad, op_only_d_params=d["params"].grad,
                   op_only_d_grids=[t.grad for t in as_list(d["grid"])])
        return res

    check_guarded(f"points {name}", run, ("op", "col", "d_points", "op_only", "op_only_d_points"), expect=("opacity", "color", "d_points"))


# ---- gather and splat at points -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PG.CASES))
def test_gather_and_splat(name):
    dev, c = _dev(), PG.case(name)
    from tests.test_gpu_point_grid import _as_list, _gather, _splat

    def run():
        grid, sizes = PG.grid_arg(c, c["grids"], dev, requires_grad=True)
        pts = c["pts"].to(dev).requires_grad_(True)
        out = _gather(c, grid, sizes, pts)
        d_grids = torch.autograd.grad(out, _as_list(grid), c["vec"].to(dev), retain_graph=True)
        (d_pts,) = torch.autograd.grad(out, pts, c["vec_live"].to(dev))
        res = dict(gather=out.detach(), gather_d_grids=list(d_grids), gather_d_points=d_pts)
        ups = [u.to(dev) for u in PG.in_form(c, c["up_grids"])]
        for normalize, key in ((False, "raw"), (True, "norm")):
            feat = c["vec"].to(dev).requires_grad_(True)
            outs = _splat(c, c["pts"].to(dev), feat, normalize)
            sum((o * u).sum() for o, u in zip(outs, ups)).backward()
            res[f"splat_{key}"] = [o.detach() for o in outs]
            res[f"splat_{key}_d_features"] = feat.grad
        pts = c["pts"].to(dev).requires_grad_(True)
        outs = _splat(c, pts, c["vec_live"].to(dev), False)
        sum((o * u).sum() for o, u in zip(outs, ups)).backward()
        res["splat_raw_d_points"] = pts.grad
        return res

    # (the normalised splat's backward divides by the splatted weights, which atomics accumulate: within the bar, not bit for bit)
    check_guarded(f"point-grid {name}", run, ("gather", "gather_d_points", "splat_raw_d_features", "splat_raw_d_points"),
                  expect=("out", "d_points", "d_features"))


# ---- resampling ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [4, 5])
@pytest.mark.parametrize("shape_key", list(RS.SHAPES))
def test_resample(shape_key, C):
    """every mapping, both containers, forward and adjoint (align_corners off and on); C = 4 and 5 are new here: the unguarded baseline
    is held to the fp64 definition (RS.ref_resample) first"""
    for mapping in RS.MAPPINGS:
        for align in (False, True):
            xs, gys, out_dhw, scale, ref_y, ref_gx = RS._case(shape_key, C, align, mapping)
            for flat in (False, True):
                tag = f"resample {shape_key} C={C} {mapping} {'ac' if align else 'nac'} {'flat' if flat else 'list'}"

                def run():
                    ys, gxs = RS._run(xs, gys, out_dhw, scale, align, flat)
                    return dict(y=[y.detach() for y in ys], gx=gxs)

                base, _ = check_guarded(tag, run, ("y", "gx"), expect=("outs", "grads"))
                for k, (y, r) in enumerate(zip(base["y"], ref_y)):
                    _assert_close(f"{tag} out[{k}]", y, r)
                for k, (g, r) in enumerate(zip(base["gx"], ref_gx)):
                    _assert_close(f"{tag} grad[{k}]", g, r)


# ---- total variation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("kind", list(TV.SHAPES))
def test_grid_tv(kind, p):
    """C = 16 (a row of tests/test_gpu_grid_tv.py::test_sweep_matches_the_fp64_definition), list and flat; no atomics: the loss, the
    gradient and the fused sweep's sums are the baseline's bit for bit with a poisoned workspace -- the second of two runs as well"""
    dev = _dev()
    C = 16
    host = TV._random_grids(TV.SHAPES[kind], C, seed=C + p)
    for flat in (False, True):
        def run():
            if flat:
                x = torch.cat([g.reshape(-1, C) for g in host]).to(dev).requires_grad_(True)
                sizes = [list(g.shape) for g in host]
                loss = lp.grid_tv_loss(x, grid_sizes=sizes, p=p)
                loss.backward()
                buf = torch.zeros_like(x)
                fused = lp.add_grid_tv_grad_(x.detach(), buf, weight=0.5, p=p, grid_sizes=sizes)
                return dict(loss=loss.detach(), grad=[x.grad], fused=fused, bufs=[buf])
            xs = [g.to(dev).requires_grad_(True) for g in host]
            loss = lp.grid_tv_loss(xs, p=p)
            loss.backward()
            bufs = [torch.zeros_like(t) for t in xs]
            fused = lp.add_grid_tv_grad_([t.detach() for t in xs], bufs, weight=0.5, p=p)
            return dict(loss=loss.detach(), grad=[t.grad for t in xs], fused=fused, bufs=bufs)

        def twice():
            a, b = run(), run()
            return dict(first=a, second=b)

        base, _ = check_guarded(f"grid-tv {kind} p={p} {'flat' if flat else 'list'}", twice, ("first", "second"), expect=("workspace", "loss", "grads"))
        _compare(f"grid-tv {kind} p={p}: the second run", base["second"], base["first"], ("loss", "grad", "fused", "bufs"))


# ---- scaffold ------------------------------------------------------------------------------------------------------------------------
SCAFFOLD_CASE = "triplane_c16_22x32_r1"   # [2, 6, 5, 7]: the smallest lattice of tests/test_gpu_scaffold.py with unequal axes and B = 2


def test_scaffold():
    dev, c = _dev(), SC._case(SCAFFOLD_CASE)
    assert c["size"][0] == 2 and len(set(c["size"][1:])) == 3

    def run():
        grid, sizes, dec = SC._on(dev, c)
        res = dict(opacity=lp.scaffold_opacity(grid, dec, c["size"], gain=SC.GAIN, mask_out_of_bounds_samples=c["mask"], grid_sizes=sizes))
        for r in (0, 2):
            res[f"dilate{r}"] = lp.calculate_scaffold(grid, dec, c["size"], gain=SC.GAIN, threshold=c["t"], dilate_scaffold=r,
                                                      mask_out_of_bounds_samples=c["mask"], grid_sizes=sizes)
        return res

    base, _ = check_guarded("scaffold", run, ("opacity", "dilate0", "dilate2"), expect=("workspace",))
    _assert_close("scaffold opacity", base["opacity"], c["op"])
    for r in (0, 2):   # (dilate 2 is new here: exact against the oracle's occupancy, as test_every_dilation_radius_on_one_lattice asks)
        assert torch.equal(base[f"dilate{r}"].cpu(), SC.oracle_occupancy(c["op"], c["t"], r)), f"dilate {r}"


# ---- ray clip ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RC.CASE_NAMES)
def test_ray_clip(name):
    """rays without a hit, with far < near, NaN rays and rays with grid_idx out of range 'keep their near / far bit for bit': under poison
    a statement about the OUTPUT buffers"""
    dev, c = _dev(), RC.case(name)
    rays = lp.Rays(directions=c["d"].to(dev), origins=c["o"].to(dev), grid_idx=c["grid_idx"].to(dev), near=c["near"].to(dev), far=c["far"].to(dev),
                   encoding=None)
    scaffold = None if c["scaffold"] is None else c["scaffold"].to(dev)

    def run():
        res = {}
        for pad in RC.PADS:
            clipped, hit = lp.clip_rays_to_scaffold(rays, scaffold, pad=pad)
            RC.check_misses(c, clipped.near.cpu(), clipped.far.cpu(), hit.cpu())
            res[f"pad{pad}"] = dict(near=clipped.near, far=clipped.far, hit=hit)
        return res

    base, _ = check_guarded(f"ray-clip {name}", run, tuple(f"pad{p}" for p in RC.PADS), expect=("near, far", "hit"))
    assert any(not bool(v["hit"].all()) for v in base.values()), "every ray hits: the case has no miss to keep"


# ---- ray embedding -------------------------------------------------------------------------------------------------------------------
def test_ray_embedding():
    dev = _dev()
    n = 160
    torch.manual_seed(5)
    mod = lp.LightplaneRenderer(num_samples=8, color_chn=3, grid_chn=16, mlp_hidden_chn=32, ray_embedding_num_harmonics=3).to(dev)
    gen = torch.Generator().manual_seed(6)
    dirs = torch.randn(n, 3, generator=gen) * torch.rand(n, 1, generator=gen) * 3.0
    up = torch.randn(n, mod.rays_encoding_dim, generator=gen)
    lin = mod.harmonic_ray_embedding_linear

    def run():
        lin.weight.grad = lin.bias.grad = None
        with config_set(fused_module_ops=True):
            out = mod._get_ray_embedding(dirs.to(dev))
            out.backward(up.to(dev))
        return dict(out=out.detach(), gw=lin.weight.grad.clone(), gb=lin.bias.grad.clone())

    base, _ = check_guarded("ray-embedding", run, ("out",), expect=("out",))
    # new here: the op chain of the reference (normalize -> harmonics -> Linear) in fp64
    from lightplane_amd.modules import calc_harmonic_embedding
    w = lin.weight.detach().cpu().double().requires_grad_(True)
    b = lin.bias.detach().cpu().double().requires_grad_(True)
    ref = torch.nn.functional.linear(calc_harmonic_embedding(torch.nn.functional.normalize(dirs.double(), dim=-1), 3), w, b)
    ref.backward(up.double())
    _assert_close("ray embedding", base["out"], ref.detach().numpy())
    _assert_close("ray embedding: grad weight", base["gw"], w.grad.numpy())
    _assert_close("ray embedding: grad bias", base["gb"], b.grad.numpy())


def test_zz_what_was_checked():
    """(runs last in this file) the totals DESIGN.md quotes"""
    print("unwritten-buffers totals: " + ", ".join(f"{k} {v:.3e}" if isinstance(v, float) else f"{k} {v}" for k, v in STATS.items())
          + f"; worst ratio / bar {STATS['worst'] / BAR:.3f}")
    if STATS["cases"]:
        assert STATS["buffers"] > 0 and STATS["fenced"] > STATS["buffers"] and STATS["worst"] <= BAR

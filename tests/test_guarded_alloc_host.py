"""The poison-and-fence harness (tests/guarded_alloc.py) can fail: plain torch code on the CPU stands in for a kernel
(``guarded(..., device="cpu")``, a switch that exists for this file only) and breaks each promise the GPU test
(tests/test_gpu_unwritten_buffers.py) checks.  No GPU, and no library for the front-end calls at the end: ``_lib.lib()`` is a stub
that returns 0, as in tests/test_layout_host.py."""
import contextlib
import dataclasses

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib
from tests import guarded_alloc as GA
from tests.guarded_alloc import PATTERNS, guarded
from tests.synth import RENDERER_CASES

DTYPES = (torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8)


def test_the_pattern_set():
    """At least four patterns; per dtype pattern 1 differs from the value the others share, and no poison is the canary."""
    assert len(PATTERNS) >= 4 and PATTERNS[0] == "nan"
    f = {p: torch.tensor([GA.poison_bits(p, torch.float32)], dtype=torch.int32).view(torch.float32).item() for p in PATTERNS}
    assert f["nan"] != f["nan"] and (f["+1e30"], f["-1e30"], f["0.5"]) == (pytest.approx(1e30), pytest.approx(-1e30), 0.5)
    d = {p: torch.tensor([GA.poison_bits(p, torch.float64)], dtype=torch.int64).view(torch.float64).item() for p in PATTERNS}
    assert d["nan"] != d["nan"] and (d["+1e30"], d["-1e30"], d["0.5"]) == (1e30, -1e30, 0.5)
    for dt in (torch.int32, torch.int64):
        assert GA.poison_bits("nan", dt) == -1 and {GA.poison_bits(p, dt) for p in PATTERNS[1:]} == {GA._INT_OTHER} != {-1}
    assert GA.poison_bits("nan", torch.uint8) == 255 and {GA.poison_bits(p, torch.uint8) for p in PATTERNS[1:]} == {GA._U8_OTHER} != {255}
    for dt in DTYPES:
        canary = torch.full((8,), GA.CANARY, dtype=torch.uint8).view(GA._BITS_VIEW[dt])[0].item()
        assert all(GA.poison_bits(p, dt) != canary for p in PATTERNS), dt
    assert GA.FENCE_BYTES == 256 and GA.FENCE_BYTES % 16 == 0


@pytest.mark.parametrize("pattern", PATTERNS)
def test_views_are_aligned_contiguous_and_of_the_requested_shape_and_dtype(pattern):
    x = torch.arange(15, dtype=torch.float32).reshape(3, 5)
    with guarded(pattern, device="cpu") as g:
        made = [torch.empty(7, dtype=torch.float32), torch.empty(3, 5, dtype=torch.float64), torch.empty((2, 3, 1), dtype=torch.uint8),
                torch.empty((), dtype=torch.float32), torch.zeros(5, dtype=torch.int32), torch.zeros((2, 2), dtype=torch.int64),
                torch.empty_like(x), torch.zeros_like(x), torch.empty_like(x, dtype=torch.uint8), torch.empty(size=(4,), dtype=torch.float32),
                torch.zeros(3, device="cpu"), torch.empty(3, requires_grad=True)]
        shapes = [(7,), (3, 5), (2, 3, 1), (), (5,), (2, 2), (3, 5), (3, 5), (3, 5), (4,), (3,), (3,)]
        dtypes = [torch.float32, torch.float64, torch.uint8, torch.float32, torch.int32, torch.int64, torch.float32, torch.float32,
                  torch.uint8, torch.float32, torch.float32, torch.float32]
        assert len(g.records) == len(made)
        for t, r, s, dt in zip(made, g.records, shapes, dtypes):
            assert tuple(t.shape) == s == r.shape and t.dtype == dt == r.dtype and t.is_contiguous()
            assert t.data_ptr() % 16 == 0, r.where()
            assert r.fences is not None and all(f.numel() == GA.FENCE_BYTES and bool((f == GA.CANARY).all()) for f in r.fences)
            assert r.fences[0].data_ptr() + GA.FENCE_BYTES == t.data_ptr() and r.fences[1].data_ptr() == t.data_ptr() + t.numel() * t.element_size()
            assert r.site[0] == __file__ and r.payload.data_ptr() == t.data_ptr()
            if r.fn.startswith("zeros"):
                assert not r.poisoned and int(t.detach().count_nonzero()) == 0
            else:
                assert r.poisoned and g.unwritten(r) == t.numel()
        assert made[-1].requires_grad and g.records[0].name == "made"
        # what the harness leaves alone: other dtypes, out=, a non-contiguous memory format, another device type; zero elements are
        # forwarded, but on the ledger
        n = len(g.records)
        torch.empty(3, dtype=torch.float16), torch.zeros(3, dtype=torch.bool), torch.empty(4, out=torch.ones(4))
        torch.empty(2, 3, 4, 5, memory_format=torch.channels_last), torch.empty_like(x.t()), torch.empty(3, device="meta")
        assert len(g.records) == n
        e = torch.empty(0, 3, dtype=torch.float32)
        assert len(g.records) == n + 1 and g.records[-1].fences is None and e.shape == (0, 3) and not g.records[-1].poisoned
    assert (made[0] != made[0]).all() if pattern == "nan" else (made[0] == float(pattern)).all()


def test_the_four_functions_are_restored_after_an_exception():
    real = [getattr(torch, n) for n in GA._NAMES]
    with pytest.raises(ZeroDivisionError):
        with guarded("nan", device="cpu"):
            assert all(getattr(torch, n) is not r for n, r in zip(GA._NAMES, real))
            1 / 0
    assert all(getattr(torch, n) is r for n, r in zip(GA._NAMES, real))
    with guarded("0.5", device="cpu"):
        pass
    assert all(getattr(torch, n) is r for n, r in zip(GA._NAMES, real))


def test_the_replacement_is_seen_from_another_thread():
    """The autograd engine runs a backward on its own thread: the module attribute is what is patched."""
    import threading
    seen = []
    with guarded("+1e30", device="cpu") as g:
        t = threading.Thread(target=lambda: seen.append(torch.empty(3)))
        t.start()
        t.join()
        assert len(g.records) == 1 and g.unwritten(g.records[0]) == 3
    assert (seen[0] == 1e30).all()


# ---- (a) one element left unwritten ---------------------------------------------------------------------------------------------
def _kernel_with_a_forgotten_tail(n, skip):
    """Stands in for a kernel that "writes" its result and forgets element ``skip``."""
    out = torch.empty(n, dtype=torch.float32)
    vals = torch.linspace(1.0, 2.0, n)
    keep = torch.ones(n, dtype=torch.bool)
    if skip is not None:
        keep[skip] = False
    out[keep] = vals[keep]
    return out


@pytest.mark.parametrize("pattern", PATTERNS)
def test_one_unwritten_element_is_reported_under_every_pattern(pattern):
    with guarded(pattern, device="cpu") as g:
        _kernel_with_a_forgotten_tail(37, None)
        _kernel_with_a_forgotten_tail(37, 36)
    full, short = g.from_file("test_guarded_alloc_host.py")
    assert full.name == short.name == "out"
    assert g.unwritten(full) == 0
    assert g.unwritten(short) == 1 and g.unwritten_mask(short).nonzero().flatten().tolist() == [36]
    for dt in (torch.float64, torch.int32, torch.int64, torch.uint8):
        with guarded(pattern, device="cpu") as g:
            buf = torch.empty(9, dtype=dt)
            buf[:8] = 1
        assert g.unwritten(g.records[0]) == 1, dt


# ---- (b) a store one element outside the payload ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", ["empty", "zeros", "empty_like", "zeros_like"])
@pytest.mark.parametrize("where", ["before", "behind"])
def test_a_store_one_element_outside_the_payload_is_reported(fn, where):
    like = torch.ones(6, 4)
    with pytest.raises(AssertionError) as info:
        with guarded("nan", device="cpu") as g:
            make = getattr(torch, fn)
            t = make(like) if fn.endswith("_like") else make(6, 4, dtype=torch.float32)
            g.check()   # nothing touched yet
            # a scatter whose row index is off by one: element -1 / element numel of the buffer
            flat = torch.as_strided(t, (1,), (1,), t.storage_offset() + (-1 if where == "before" else t.numel()))
            flat[0] = 3.0
    msg = str(info.value)
    assert f"fence {where} the payload" in msg and "test_guarded_alloc_host.py" in msg and f"torch.{fn}" in msg
    assert ("byte offset -4 " if where == "before" else "byte offset +0 ") in msg, msg
    assert "(4 of 256 bytes)" in msg and "shape (6, 4)" in msg


def test_a_store_of_the_canary_value_itself_is_the_only_blind_spot():
    """Bit-identical means bit-identical: any other byte shows."""
    with guarded("0.5", device="cpu") as g:
        t = torch.empty(4, dtype=torch.uint8)
        beyond = torch.as_strided(t, (1,), (1,), t.storage_offset() + 4)
        beyond[0] = GA.CANARY
        assert g.fence_failures() == []
        beyond[0] = GA.CANARY ^ 1
        assert len(g.fence_failures()) == 1
        beyond[0] = GA.CANARY


# ---- (c) a consumer that clamps: NaN alone is not enough --------------------------------------------------------------------------
def _forward_that_forgets_the_last_checkpoint(x):
    """The "forward": running sums of ``x`` per block of 4, the last (partial) block's checkpoint is never stored."""
    n_blk = (x.numel() + 3) // 4
    ckpt = torch.empty(n_blk, dtype=torch.float32)
    for b in range(n_blk - 1):
        ckpt[b] = x[: 4 * (b + 1)].sum()
    return ckpt


def _backward_that_clamps(ckpt):
    """The "backward": reads every checkpoint and clamps as the tuned backward does behind its checkpoint read,
    ``if (!(nlt > 0.0f)) nlt = 0`` -- a NaN and any negative value become 0."""
    nlt = ckpt.clone()
    nlt[~(nlt > 0.0)] = 0.0
    return torch.exp(-nlt).sum()


def test_a_clamping_consumer_swallows_nan_and_is_caught_by_the_pattern_set():
    x = torch.linspace(0.1, 0.3, 10)
    results = {}
    unwritten = {}
    for p in PATTERNS:
        with guarded(p, device="cpu") as g:
            results[p] = float(_backward_that_clamps(_forward_that_forgets_the_last_checkpoint(x)))
        unwritten[p] = g.unwritten(g.records[0])
    # the ledger sees the hole under every pattern ...
    assert all(v == 1 for v in unwritten.values()), unwritten
    # ... but a comparison of RESULTS does not: the value a zero-filled (fresh) block would give is the "baseline" a lucky test sees
    lucky = torch.zeros(3)
    lucky[:2] = _forward_that_forgets_the_last_checkpoint(x)[:2]
    baseline = float(_backward_that_clamps(lucky))
    differs = {p: abs(results[p] - baseline) > 2e-5 * abs(baseline) for p in PATTERNS}
    assert differs["nan"] is False, "the clamp turns the NaN into the 0 a fresh block holds: pattern 1 alone misses the bug"
    assert differs["-1e30"] is False, "... and any negative garbage as well"
    assert differs["+1e30"] is True and differs["0.5"] is True, differs
    assert any(differs.values()) and not all(differs.values())


# ---- the ledger sees the front-ends' allocations -----------------------------------------------------------------------------------
class _Zero:
    """Stands in for the loaded library: every entry point returns 0 (tests/test_layout_host.py: _Recorder)."""

    def __getattr__(self, name):
        return lambda *args: 0


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: _Zero())
    monkeypatch.setattr(_lib, "current_stream", lambda dev: None)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())


def _by_name(records):
    out = {}
    for r in records:
        out.setdefault((r.fn, r.name), []).append(r)
    return {k: len(v) for k, v in out.items()}


@pytest.mark.filterwarnings("ignore:lightplane_amd")
def test_the_ledger_counts_the_renderers_buffers(no_library):
    """renderer.py: ray_length, nlt, feature, alpha (zero elements without the module epilogue: forwarded, recorded), ckpt in the
    forward -- no segment records and no workspace, the stub answers 0 segments / 0 bytes --; one zeros_like per grid tensor, one for
    mlp_params and one for the encoding in the backward."""
    case = dataclasses.replace(next(c for c in RENDERER_CASES if c.name == "triplane_basic"), n_rays=5)
    d = case.build()
    rays = d["rays"]
    rays.encoding = rays.encoding.clone().requires_grad_(True)
    dec = d["decoder"]
    hdec = lp.DecoderParams(dec.mlp_params.clone().requires_grad_(True), dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
    grids = [g.clone().requires_grad_(True) for g in d["grids"]]
    cfg = d["cfg"]
    with guarded("nan", device="cpu") as g:
        out = lp.lightplane_renderer(rays, grids, hdec, **cfg)
        torch.autograd.backward(list(out), [torch.ones_like(o) for o in out])
    recs = g.from_file("lightplane_amd/renderer.py")
    n = 5
    n_ckpt = _lib.n_nlt_ckpt(cfg["num_samples"], cfg["num_samples_inf"])
    assert _by_name(recs) == {("empty", "ray_length"): 1, ("empty", "nlt"): 1, ("empty", "feature"): 1, ("empty", "alpha"): 1, ("empty", "ckpt"): 1,
                              ("zeros_like", "grad_grids"): len(grids), ("zeros_like", "grad_params"): 1, ("zeros_like", "grad_enc"): 1}
    shapes = {r.name: r.shape for r in recs if r.fn == "empty"}
    assert shapes == {"ray_length": (n,), "nlt": (n,), "feature": (n, dec.color_chn), "alpha": (0,), "ckpt": (n, n_ckpt)}
    # the stub wrote nothing: every poisoned element is still poison, the gradient buffers are the zeros the caller fills in
    for r in recs:
        if r.poisoned:
            assert g.unwritten(r) == r.payload.numel(), r.where()
    assert all(float(t.grad.abs().max()) == 0.0 for t in grids) and hdec.mlp_params.grad.abs().max() == 0
    assert out[0].data_ptr() % 16 == 0 and bool((out[0] != out[0]).all())


def test_the_ledger_counts_the_tv_buffers(no_library):
    """regularizers.py: the fp64 workspace and the loss in the forward, one empty_like gradient per grid in the backward; the fused sweep
    allocates the workspace and the loss alone."""
    xs = [torch.randn(2, 1, 4, 3, 5).requires_grad_(True), torch.randn(2, 4, 1, 3, 5).requires_grad_(True), torch.randn(2, 4, 3, 1, 5).requires_grad_(True)]
    with guarded("-1e30", device="cpu") as g:
        lp.grid_tv_loss(xs, p=1).backward()
    recs = g.from_file("lightplane_amd/regularizers.py")
    assert _by_name(recs) == {("empty", "workspace"): 1, ("empty", "loss"): 1, ("empty_like", "grads"): 3}
    assert [r.dtype for r in recs[:2]] == [torch.float64, torch.float32] and recs[1].shape == ()
    assert [r.shape for r in recs[2:]] == [tuple(t.shape) for t in xs]
    bufs = [torch.zeros_like(t) for t in xs]
    with guarded("-1e30", device="cpu") as g:
        lp.add_grid_tv_grad_([t.detach() for t in xs], bufs)
    assert _by_name(g.from_file("lightplane_amd/regularizers.py")) == {("empty", "workspace"): 1, ("empty", "loss"): 1}


def test_the_ledger_counts_the_ray_clips_buffers(no_library):
    """ray_clip.py: near, far (one line, two empty_like) and the uint8 hit flags."""
    n = 9
    rays = lp.Rays(directions=torch.randn(n, 3), origins=torch.randn(n, 3), grid_idx=torch.zeros(n, dtype=torch.int32), near=torch.zeros(n),
                   far=torch.ones(n), encoding=None)
    with guarded("0.5", device="cpu") as g:
        clipped, hit = lp.clip_rays_to_scaffold(rays, torch.ones(1, 2, 2, 2))
    recs = g.from_file("lightplane_amd/ray_clip.py")
    assert _by_name(recs) == {("empty_like", "near, far"): 2, ("empty", "hit"): 1}
    assert [r.dtype for r in recs] == [torch.float32, torch.float32, torch.uint8] and all(r.shape == (n,) for r in recs)
    assert bool((clipped.near == 0.5).all()) and bool((clipped.far == 0.5).all()) and bool(hit.all())

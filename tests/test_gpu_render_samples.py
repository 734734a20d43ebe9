"""``lightplane_amd.render_samples`` (csrc/lp_render_samples.hip) against its fp64 definition and against the chain it replaces.

Cases, regimes and the definition: tests/render_samples_cases.py (tests/test_render_samples_host.py checks them without a GPU).  The
depths come from the library's own sample ops on the GPU, so the chain

    ray_samples | importance_samples -> lightplane_eval_mlp(.points) -> composite_samples(return_weights=True)

decodes bit-identical points.  Bars: the project's ``TOL`` (1e-4 of max |ref| per tensor) against fp64 and for the chain's three
reductions and gradients; 1e-6 of max |ref| for the weights against the chain (same decode body, same scan: bit-identity is expected and
printed; the bar admits last-bit contraction differences between translation units, a wrong sample or delta is >= 1e-3); 2e-5 for
atomically accumulated gradients of the same kernel on the same inputs (tests/test_gpu_partial_grads.py).  Every figure is printed
before it is asserted.  References are computed once per process and never modified."""
import ctypes
import itertools
import json
import os
import subprocess
import sys

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib
from tests import compositing_cases as CC
from tests import guarded_alloc as GA
from tests import points_cases as PC
from tests import render_samples_cases as RC
from tests.test_gpu_parity import _dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = RC.TOL
W_BAR = 1e-6
ATOMIC_BAR = 2e-5
PLAIN = [c for c in RC.CASES if not RC.scene(c[0])["jumps"]]
LEAVES = ("grids", "cgrids", "params", "enc")
_SAMPLES, _REF, _CHAIN = {}, {}, {}


def _worst(name, got, want, tol=TOL):
    """max |err| / max |ref| over every entry, printed and held to the bar"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    assert bool(torch.isfinite(got).all()), f"{name}: not finite"
    scale = max(float(want.abs().max()), 1e-30)
    err = float((got - want).abs().max()) / scale
    print(f"{name}: max |err| / max |ref| = {err:.3e} (max |ref| {scale:.4g})")
    assert err <= tol, f"{name}: {err:.3e} > {tol}"
    return err


def _rays(name, R, dev):
    r = RC.rays_for(name, R)
    return lp.Rays(directions=r.directions.to(dev), origins=r.origins.to(dev), grid_idx=r.grid_idx.to(dev).to(torch.int32), near=r.near.to(dev),
                   far=r.far.to(dev), encoding=r.encoding.to(dev))


def _scene_on(sc, dev, requires_grad=()):
    """the scene's tensors on the device in its grid form (points_cases.on_device), leaves made to require a gradient"""
    stub = dict(sc, pts=torch.zeros(1, 1, 3), gidx=torch.zeros(1, dtype=torch.long), enc=torch.zeros(1, sc["enc_dim"]))
    return PC.on_device(stub, dev, requires_grad)


def samples_of(c, dev):
    """(RaySamples on the device, gain) of a case: the depths of its regime from the library's sample ops, built once"""
    if c in _SAMPLES:
        return _SAMPLES[c]
    name, R, S, depth, opac = c
    sc, rays = RC.scene(name), _rays(name, R, dev)
    a, b = RC.split_samples(S, depth)
    with torch.no_grad():
        if depth == "resampled":
            coarse = lp.ray_samples(rays, a)
            s = lp.importance_samples(rays, RC.peaked_depths(coarse.depths), RC.peaked_weights(R, a).to(dev), b)
        else:
            s = lp.ray_samples(rays, a, b, disparity_at_inf=RC.DISPARITY)
        if depth == "zero":
            s = lp.RaySamples(s.points, s.depths, torch.zeros_like(s.deltas))
    assert s.depths.shape == (R, S)
    gain = RC.gain_for(sc, RC.rays_for(name, R), s.depths.cpu(), s.deltas.cpu(), RC.contract_of(c), opac)
    _SAMPLES[c] = (s, gain)
    return _SAMPLES[c]


def _call(c, dev, d, rays, s, gain, return_weights=True):
    sc = RC.scene(c[0])
    return lp.render_samples(rays, s.depths, s.deltas, d["grid"], d["dec"], gain=gain, mask_out_of_bounds_samples=sc["mask"],
                             contract_coords=RC.contract_of(c), scaffold=d["scaffold"], color_grid=d["color_grid"], grid_sizes=d["sizes"],
                             color_grid_sizes=d["color_sizes"], return_weights=return_weights)


def _chain(c, dev, d, rays, s, gain):
    sc = RC.scene(c[0])
    opacity, color = lp.lightplane_eval_mlp(s.points, d["grid"], rays.grid_idx, d["dec"], rays.encoding, gain, sc["mask"], None, d["scaffold"],
                                            d["color_grid"], RC.contract_of(c), grid_sizes=d["sizes"], color_grid_sizes=d["color_sizes"])
    return lp.composite_samples(opacity, color, s.depths, s.deltas, return_weights=True)


def _ups(c, dev):
    gen = torch.Generator().manual_seed(31 + 1000 * c[1] + 7 * c[2] + list(RC.SHAPES).index(c[0]))
    R, S = c[1], c[2]
    return [torch.randn(R, generator=gen).to(dev), torch.randn(R, generator=gen).to(dev), torch.randn(R, 3, generator=gen).to(dev),
            torch.randn(R, S, generator=gen).to(dev)]


def _leaf_grads(d, rays):
    def grads(x):
        return [] if x is None else [t.grad for t in (x if isinstance(x, (list, tuple)) else [x])]
    return dict(grids=grads(d["grid"]), cgrids=grads(d["color_grid"]), params=[d["params"].grad], enc=[rays.encoding.grad])


def _run(c, dev, leaves=LEAVES, upstream=(0, 1, 2, 3), fn=_call):
    """forward + backward with the named leaves requiring a gradient and the numbered results in the loss: (results, gradients)"""
    s, gain = samples_of(c, dev)
    d = _scene_on(RC.scene(c[0]), dev, tuple(k for k in leaves if k != "enc"))
    rays = _rays(c[0], c[1], dev)
    if "enc" in leaves:
        rays.encoding.requires_grad_(True)
    out = fn(c, dev, d, rays, s, gain)
    ups = _ups(c, dev)
    if upstream and leaves:
        sum((out[i] * ups[i]).sum() for i in upstream).backward()
    return tuple(o.detach() for o in out), _leaf_grads(d, rays)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. values against the fp64 definition
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", PLAIN, ids=RC.case_id)
def test_values_against_fp64(c):
    dev = _dev()
    name, R, S, depth, opac = c
    s, gain = samples_of(c, dev)
    if c not in _REF:
        with torch.no_grad():
            _REF[c] = RC.definition(RC.scene(name), RC.rays_for(name, R), s.depths.cpu().double(), s.deltas.cpu().double(), gain,
                                    RC.contract_of(c))
    want = _REF[c]
    with torch.no_grad():
        got = _call(c, dev, _scene_on(RC.scene(name), dev), _rays(name, R, dev), s, gain)
    print(f"{RC.case_id(c)}: gain {gain:.4g}, median -log T {float(want[1].median()):.4g}, delta range "
          f"[{float(s.deltas.min()):.3g}, {float(s.deltas.max()):.3g}], zero deltas {int((s.deltas == 0).sum())}")
    if depth == "resampled" and S >= 63:
        assert int((s.deltas == 0).sum()) > 0, "the peaked weight row gave no run of equal depths"
    if opac == "opaque" and depth != "zero" and S >= 63:
        assert bool((torch.exp(-want[1].float()) == 0).any()), "no ray's T underflows in fp32"
    for key, g, w in zip(("ray_length", "neg_log_t", "feature", "weights"), got, want):
        _worst(f"{RC.case_id(c)} {key}", g, w)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. / 3. values and gradients against the chain on the GPU
# ------------------------------------------------------------------------------------------------------------------------------

def _chain_of(c, dev):
    if c not in _CHAIN:
        _CHAIN[c] = _run(c, dev, fn=_chain)
    return _CHAIN[c]


@pytest.mark.parametrize("c", RC.CASES, ids=RC.case_id)
def test_values_and_gradients_against_the_chain(c):
    dev = _dev()
    want, want_g = _chain_of(c, dev)
    got, got_g = _run(c, dev)
    print(f"{RC.case_id(c)}: weights bit-identical to the chain's: {torch.equal(got[3], want[3])}; all four results: "
          f"{all(torch.equal(a, b) for a, b in zip(got, want))}")
    _worst(f"{RC.case_id(c)} weights vs chain", got[3], want[3], tol=W_BAR)
    for key, g, w in zip(("ray_length", "neg_log_t", "feature"), got, want):
        _worst(f"{RC.case_id(c)} {key} vs chain", g, w)
    worst = 0.0
    for k in LEAVES:
        assert len(got_g[k]) == len(want_g[k])
        for i, (g, w) in enumerate(zip(got_g[k], want_g[k])):
            assert g is not None and w is not None, (k, i)
            worst = max(worst, _worst(f"{RC.case_id(c)} d {k}[{i}] vs chain", g, w))
    print(f"{RC.case_id(c)}: worst gradient ratio {worst:.3e}")


# ------------------------------------------------------------------------------------------------------------------------------
# 4. gradients against fp64: the chain's own cases
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CC.CHAIN_CASES))
def test_gradients_against_fp64(name):
    dev, c = _dev(), CC.chain_case(name)
    r = c["rays"]
    rays = lp.Rays(**{k: getattr(r, k).to(dev) for k in ("origins", "directions", "near", "far", "grid_idx", "encoding")})
    grids = [g.to(dev).requires_grad_(True) for g in c["grids"]]
    dec = lp.DecoderParams(c["dec"].mlp_params.to(dev).requires_grad_(True), c["dec"].n_hidden_trunk, c["dec"].n_hidden_opacity,
                           c["dec"].n_hidden_color, 3)
    s = lp.ray_samples(rays, CC.CHAIN_S, CC.CHAIN_S_INF, disparity_at_inf=CC.CHAIN_DISPARITY)
    out = lp.render_samples(rays, s.depths.detach(), s.deltas.detach(), grids, dec, gain=CC.CHAIN_GAIN, contract_coords=c["contract"])
    for key, o, want in zip(("ray_length", "neg_log_t", "feature"), out, c["out"]):
        _worst(f"{name} {key} vs the fp64 oracle Renderer", o, want)
    sum((o * u.to(dev)).sum() for o, u in zip(out, c["ups"])).backward()
    for i, (g, want) in enumerate(zip(grids, c["grads"]["grids"])):
        _worst(f"{name} d grid[{i}]", g.grad, want)
    _worst(f"{name} d mlp_params", dec.mlp_params.grad, c["grads"]["mlp_params"])


# ------------------------------------------------------------------------------------------------------------------------------
# 5. partial gradients
# ------------------------------------------------------------------------------------------------------------------------------

def _subsets(items):
    return [s for n in range(len(items) + 1) for s in itertools.combinations(items, n)]


@pytest.mark.parametrize("c", [("voxel_c32_twogrid_022x32", 9, 65, "uniform", "mixed"), ("triplane_c16_222x32", 9, 130, "resampled", "mixed")],
                         ids=RC.case_id)
def test_partial_gradients(c):
    """every subset of the leaves x every subset of the upstream gradients: the forward and grad_encoding are those of the run with
    every leaf, bit for bit; the atomically accumulated gradients agree with it at 2e-5; a leaf outside the subset gets none"""
    dev = _dev()
    leaves_here = tuple(k for k in LEAVES if k != "cgrids" or RC.scene(c[0])["cgrids"] is not None)
    worst, runs = 0.0, 0
    for upstream in _subsets((0, 1, 2, 3)):
        base_out, base_g = _run(c, dev, leaves_here, upstream)
        for leaves in _subsets(leaves_here):
            out, g = _run(c, dev, leaves, upstream)
            runs += 1
            assert all(torch.equal(a, b) for a, b in zip(out, base_out)), (leaves, upstream)
            for k in leaves_here:
                for i, (got, want) in enumerate(zip(g[k], base_g[k])):
                    if k not in leaves or not upstream:
                        assert got is None, (k, leaves, upstream)
                        continue
                    assert got is not None and bool(torch.isfinite(got).all()), (k, leaves, upstream)
                    if k == "enc":
                        assert torch.equal(got, want), (leaves, upstream)
                    else:
                        scale = max(float(want.abs().max()), 1e-30)
                        ratio = float((got.double() - want.double()).abs().max()) / scale
                        worst = max(worst, ratio)
                        assert ratio <= ATOMIC_BAR, (k, i, leaves, upstream, ratio)
    print(f"{RC.case_id(c)}: {runs} (leaves, upstreams) runs, worst ratio of an accumulated gradient to the all-leaves run {worst:.3e}")


# ------------------------------------------------------------------------------------------------------------------------------
# 6. reproducibility, graph capture
# ------------------------------------------------------------------------------------------------------------------------------

def test_two_runs_are_bit_identical():
    dev = _dev()
    for c in (("triplane_c16_222x128", 130, 200, "resampled", "mixed"), ("voxel_c32_twogrid_022x32", 130, 200, "uniform", "mixed"),
              ("triplane_c16_322x64_contract_mask_scaffold", 130, 130, "beyond_far", "opaque")):
        (o1, g1), (o2, g2) = _run(c, dev), _run(c, dev)
        assert all(torch.equal(a, b) for a, b in zip(o1, o2)), c
        assert torch.equal(g1["enc"][0], g2["enc"][0]), c
        for k in ("grids", "cgrids", "params"):
            for a, b in zip(g1[k], g2[k]):
                _worst(f"{RC.case_id(c)} d {k}: second run vs first", a, b, tol=ATOMIC_BAR)


def test_graph_capture_forward_and_backward():
    """forward + backward captured once and replayed after the inputs changed in place: the forward and grad_encoding equal the eager
    run on the same values to the bit, the atomically accumulated gradients at 2e-5"""
    dev = _dev()
    c = ("triplane_c16_222x32", 130, 130, "resampled", "mixed")
    s, gain = samples_of(c, dev)
    s = lp.RaySamples(s.points, s.depths.clone(), s.deltas.clone())
    d = _scene_on(RC.scene(c[0]), dev, ("grids", "params"))
    rays = _rays(c[0], c[1], dev)
    rays.encoding.requires_grad_(True)
    leaves = list(d["grid"]) + [d["params"], rays.encoding]
    ups = _ups(c, dev)

    def step():
        for t in leaves:
            t.grad = None
        out = _call(c, dev, d, rays, s, gain)
        sum((o * u).sum() for o, u in zip(out, ups)).backward()
        return out

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for t in leaves:
        t.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    captured = [t.grad for t in leaves]
    gen = torch.Generator().manual_seed(77)
    first = None
    for round_ in range(2):
        if round_ == 1:  # new values in the tensors the graph reads
            with torch.no_grad():
                s.depths.mul_(0.9)
                d["grid"][0].add_(0.1 * torch.randn(d["grid"][0].shape, generator=gen).to(dev))
                rays.encoding.add_(0.1)
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.detach().clone() for t in tuple(out) + tuple(captured)]
        eager = [t.detach() for t in tuple(step()) + tuple(t.grad for t in leaves)]
        for i, (a, b) in enumerate(zip(replayed, eager)):
            if i < 4 or i == len(replayed) - 1:   # the four results, grad_encoding
                assert torch.equal(a, b), f"round {round_}: replayed tensor {i} != eager"
            else:
                _worst(f"round {round_}: replayed gradient {i} vs eager", a, b, tol=ATOMIC_BAR)
        if round_ == 0:
            first = replayed[0].clone()
    assert float((replayed[0] - first).abs().max()) > 1e-4  # (the second round really saw other values)


# ------------------------------------------------------------------------------------------------------------------------------
# 7. boundary
# ------------------------------------------------------------------------------------------------------------------------------

def test_layouts_of_depths_and_deltas():
    dev = _dev()
    c = ("triplane_c16_222x32", 9, 65, "uniform", "mixed")
    s, gain = samples_of(c, dev)
    d, rays = _scene_on(RC.scene(c[0]), dev), _rays(c[0], c[1], dev)
    with torch.no_grad():
        want = _call(c, dev, d, rays, s, gain)
        transposed = lp.RaySamples(s.points, s.depths.t().contiguous().t(), s.deltas.t().contiguous().t())
        wide = torch.zeros(9, 2 * 65 + 3, device=dev)
        wide[:, 1:131:2], wide[:, 2:132:2] = s.depths, s.deltas
        sliced = lp.RaySamples(s.points, wide[:, 1:131:2], wide[:, 2:132:2])
        offset = torch.zeros(9 * 65 + 1, device=dev)
        offset[1:] = s.depths.reshape(-1)
        shifted = lp.RaySamples(s.points, offset[1:].view(9, 65), s.deltas)   # dense, but 4 bytes off a 16-byte boundary
        for what, v in (("transposed", transposed), ("sliced", sliced), ("shifted", shifted)):
            assert what == "shifted" or not v.depths.is_contiguous()
            got = _call(c, dev, d, rays, v, gain)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), what


def test_an_under_aligned_pointer_is_refused_by_the_c_abi():
    dev = _dev()
    c = ("triplane_c16_222x32", 9, 65, "uniform", "mixed")
    s, gain = samples_of(c, dev)
    sc = RC.scene(c[0])
    d, rays = _scene_on(sc, dev), _rays(c[0], c[1], dev)
    RSM = sys.modules["lightplane_amd.render_samples"]
    from lightplane_amd.grids import GridForm
    from lightplane_amd.params import int_list_of
    grids, gform = GridForm.of(d["grid"], None, name="grid", sampler=False)
    dec = d["dec"]
    cfg = RSM._Cfg(gform, None, *(tuple(int_list_of(v)) for v in (dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color)), 3, gain,
                   False, False, True)
    buf = torch.zeros(9 * 65 + 4, device=dev)
    for field in ("depths", "deltas", "weights", "chunk_nlt"):
        a = RSM._fill(cfg, rays.origins, rays.directions, rays.grid_idx, rays.encoding, s.depths, s.deltas, dec.mlp_params, None, grids, ())
        setattr(a, field, buf.data_ptr() + 4)
        rc = _lib.lib().lp_render_samples_forward(ctypes.byref(a), None)
        msg = _lib.lib().lp_last_error().decode()
        assert rc == -1 and msg.startswith(f"{field} = ") and "16-byte aligned" in msg, (field, rc, msg)
        with pytest.raises(AssertionError, match="16-byte aligned"):
            _lib.check(rc, "lp_render_samples_forward")


def test_malformed_arguments_raise_with_their_name():
    dev = _dev()
    c = ("triplane_c16_222x32", 9, 65, "uniform", "mixed")
    s, gain = samples_of(c, dev)
    sc = RC.scene(c[0])
    d, rays = _scene_on(sc, dev), _rays(c[0], c[1], dev)
    call = lambda dp=s.depths, dl=s.deltas, r=rays: lp.render_samples(r, dp, dl, d["grid"], d["dec"], gain=gain)  # noqa: E731
    with pytest.raises(AssertionError, match="depths"):
        call(dp=s.depths[0])
    with pytest.raises(AssertionError, match="deltas"):
        call(dl=s.deltas[:, :64])
    with pytest.raises(AssertionError, match="depths has to be float32"):
        call(dp=s.depths.double())
    with pytest.raises(AssertionError, match="deltas has to be float32"):
        call(dl=s.deltas.half())
    with pytest.raises(AssertionError, match="depths is on cpu"):
        call(dp=s.depths.cpu())
    with pytest.raises(AssertionError, match="deltas is on cpu"):
        call(dl=s.deltas.cpu())
    huge = torch.zeros(1, 1, device=dev).expand(1 << 16, 1 << 15)   # R S = 2^31: shapes only, nothing is allocated
    before = torch.cuda.memory_allocated(dev)
    with pytest.raises(AssertionError, match=r"depths.*2\^31"):
        lp.render_samples(rays, huge, huge, d["grid"], d["dec"])
    assert torch.cuda.memory_allocated(dev) == before
    for what in ("depths", "deltas"):
        kw = dict(dp=s.depths, dl=s.deltas)
        kw["dp" if what == "depths" else "dl"] = getattr(s, what).clone().requires_grad_(True)
        with pytest.raises(NotImplementedError, match=rf"{what}.*\.detach\(\).*modular chain"):
            call(**kw)
        with torch.no_grad():
            call(**kw)   # (grad mode off: nothing to refuse)
    for what in ("origins", "directions"):
        r = _rays(c[0], c[1], dev)
        getattr(r, what).requires_grad_(True)
        with pytest.raises(NotImplementedError, match=rf"rays.{what}.*\.detach\(\).*modular chain"):
            call(r=r)
    torch.cuda.synchronize()


@pytest.mark.parametrize("pattern", GA.PATTERNS)
def test_every_buffer_is_written_entirely(pattern):
    """forward and backward under poisoned, fenced allocations: no element of a result, of the per-chunk -log T or of grad_encoding keeps
    the poison and every fence is intact (checked when the block ends)"""
    dev = _dev()
    with GA.guarded(pattern) as g:
        for c in (("triplane_c16_222x32", 9, 65, "uniform", "mixed"), ("voxel_c32_twogrid_022x32", 1, 65, "resampled", "opaque"),
                  ("triplane_c16_322x64_contract_mask_scaffold", 130, 130, "beyond_far", "opaque"), ("triplane_c16_222x32", 1, 1, "uniform", "mixed")):
            _run(c, dev)
            _run(c, dev, upstream=(1,))    # (no colour gradient: the colour head is not evaluated, grad_encoding is written as zeros)
            _run(c, dev, upstream=())      # (no upstream gradient: nothing runs backward)
        torch.cuda.synchronize()
        records = g.from_file("lightplane_amd/render_samples.py")
        poisoned = [r for r in records if r.poisoned]
        assert len(poisoned) >= 4 * (3 * 5 + 2), len(poisoned)
        assert {r.name for r in poisoned} >= {"length", "nlt", "feature", "weights", "chunk_nlt", "d_enc"}, {r.name for r in poisoned}
        for r in poisoned:
            assert g.unwritten(r) == 0, f"{g.unwritten(r)} of {r.payload.numel()} elements unwritten: {r.where()}"


# ------------------------------------------------------------------------------------------------------------------------------
# 8. memory
# ------------------------------------------------------------------------------------------------------------------------------

def test_memory_is_the_results_the_chunk_buffer_and_the_gradients():
    """130 rays x 200 samples, forward + backward: the peak over the baseline is at most the results, the [R, ceil(S / 64)] buffer and the
    requested gradients, each rounded up to the allocator's 512 bytes; the chain on the same inputs is printed beside it"""
    dev = _dev()
    c = ("triplane_c16_222x128", 130, 200, "resampled", "mixed")
    R, S = c[1], c[2]
    s, gain = samples_of(c, dev)
    d = _scene_on(RC.scene(c[0]), dev, ("grids", "params"))
    rays = _rays(c[0], R, dev)
    rays.encoding.requires_grad_(True)
    leaves = list(d["grid"]) + [d["params"], rays.encoding]
    ups = _ups(c, dev)

    def up512(n):
        return (n + 511) // 512 * 512

    bound = sum(up512(4 * n) for n in (R, R, 3 * R, R * S, R * ((S + 63) // 64))) + sum(up512(4 * t.numel()) for t in leaves)
    peaks = {}
    for what, fn in (("render_samples", _call), ("chain", _chain)):
        for _ in range(2):   # (the first round loads the kernels)
            for t in leaves:
                t.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            before = torch.cuda.memory_allocated(dev)
            out = fn(c, dev, d, rays, s, gain)
            # (the loss is formed by autograd.backward from the upstream gradients: no product tensors of the test's own)
            torch.autograd.backward(out, ups)
            torch.cuda.synchronize()
            peaks[what] = torch.cuda.max_memory_allocated(dev) - before
            del out
    print(f"peak memory over the baseline, forward + backward, {R} rays x {S} samples: render_samples {peaks['render_samples']} bytes "
          f"(bound {bound}), chain {peaks['chain']} bytes")
    assert peaks["render_samples"] <= bound, (peaks, bound)
    assert peaks["render_samples"] < peaks["chain"]


# ------------------------------------------------------------------------------------------------------------------------------
# 9. module and example
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("return_log_t", [False, True])
def test_the_module_is_the_function_and_the_epilogue(return_log_t):
    dev = _dev()
    torch.manual_seed(5)
    m = lp.LightplaneRenderer(num_samples=40, color_chn=3, grid_chn=16, mlp_hidden_chn=32, opacity_init_bias=-1.0, gain=1.3,
                              bg_color=(0.1, 0.5, 0.9), return_log_transmittance=return_log_t).to(dev)
    name = "triplane_c16_222x32"
    grids = [g.to(dev) for g in RC.scene(name)["grids"]]
    r = _rays(name, 130, dev)
    rays = lp.Rays(directions=r.directions, origins=r.origins, grid_idx=r.grid_idx, near=r.near, far=r.far)
    with torch.no_grad():
        coarse = m.ray_samples(rays)
        coarse = lp.RaySamples(coarse.points, RC.peaked_depths(coarse.depths), coarse.deltas)
        s = m.importance_samples(rays, coarse, RC.peaked_weights(130, 40).to(dev), 25)
        length, alpha, feature, weights = m.render_samples(rays, grids, s, return_weights=True)
        assert len(m.render_samples(rays, grids, s)) == 3
        enc = m._get_ray_encoding(None, rays.directions)
        full = lp.Rays(directions=r.directions, origins=r.origins, grid_idx=r.grid_idx, near=r.near, far=r.far, encoding=enc)
        l2, nlt, f2, w2 = lp.render_samples(full, s.depths, s.deltas, grids, m.get_decoder_params(), gain=1.3, return_weights=True)
    assert enc.shape == (130, 32)
    T = torch.exp(-nlt)
    assert torch.equal(length, l2) and torch.equal(weights, w2)
    assert torch.equal(feature, f2 + T[:, None] * m.bg_color) and torch.equal(alpha, -nlt if return_log_t else 1 - T)
    # and gradients reach the module's parameters and the planes
    planes = [g.clone().requires_grad_(True) for g in grids]
    out = m.render_samples(rays, planes, s, return_weights=True)
    (out[2].sum() + out[3].square().sum()).backward()
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in planes)
    assert all(p.grad is not None for p in m.parameters())


def test_example_fits_through_render_samples():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "fit_synthetic_scene.py"), "--modular", "--importance", "32",
                        "--render-samples", "--steps", "20", "--rays", "2048"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = r.stdout.decode()
    assert r.returncode == 0, text
    out = json.loads(text.strip().splitlines()[-1])
    print(out)
    assert out["render_samples"] is True and out["importance"] == 32 and out["steps"] == 20 and out["last_loss"] < out["first_loss"], out

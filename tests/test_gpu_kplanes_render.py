"""``lightplane_amd.kplanes_render_samples`` (csrc/lp_kplanes_render.hip) against its fp64 definition (tests/kplanes_render_cases.py)
and against the chain it replaces, ``ray_samples | importance_samples -> kplanes_eval_mlp(.points) -> composite_samples``, on depths
from the library's own sample ops.  Bar: ``TOL`` (1e-4 of max |ref| per tensor); the weights are ``torch.equal`` to the chain's.
Figures are printed before they are asserted (measured worst cases: DESIGN.md 4.27)."""
import dataclasses

import pytest
import torch

import lightplane_amd as lp
from tests import kplanes_render_cases as KC
from tests import render_samples_cases as RC
from tests.test_gpu_parity import _dev

pytestmark = pytest.mark.gpu
TOL = KC.TOL
LEAVES = ("planes", "params", "enc")
_CASES = {}


def _worst(name, got, want, tol=TOL):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape and bool(torch.isfinite(got).all()), name
    scale = max(float(want.abs().max()), 1e-30)
    err = float((got - want).abs().max()) / scale
    print(f"{name}: max |err| / max |ref| = {err:.3e} (max |ref| {scale:.4g})")
    assert err <= tol, f"{name}: {err:.3e} > {tol}"


def _rays(c, dev):
    r = c["rays"]
    return lp.Rays(**{k: getattr(r, k).to(dev) for k in ("origins", "directions", "near", "far", "encoding")}, grid_idx=r.grid_idx.to(dev).int())


def case_on(name, dev):
    if name not in _CASES:
        c = KC.inputs(name)
        rays = _rays(c, dev)
        a, b = RC.split_samples(c["S"], c["depth"])
        with torch.no_grad():
            if c["depth"] == "resampled":
                coarse = lp.ray_samples(rays, a)
                s = lp.importance_samples(rays, RC.peaked_depths(coarse.depths), RC.peaked_weights(c["R"], a).to(dev), b)
            else:
                s = lp.ray_samples(rays, a, b, disparity_at_inf=RC.DISPARITY)
        c = KC.case(name, s.depths.cpu(), s.deltas.cpu(), tag="gpu")
        _CASES[name] = (c, lp.RaySamples(s.points, s.depths, c["deltas"].to(dev)))
    return _CASES[name]


def _fused(c, d, rays, s, **kw):
    return lp.kplanes_render_samples(rays, d["times"], s.depths, s.deltas, d["planes"], c["lay"], d["dec"], gain=c["gain"],
                                     return_weights=True, **d["kw"], **kw)


def _chain(c, d, rays, s):
    opacity, color = lp.kplanes_eval_mlp(s.points, d["times"], d["planes"], rays.grid_idx, c["lay"], d["dec"], rays.encoding, c["gain"], **d["kw"])
    return lp.composite_samples(opacity, color, s.depths, s.deltas, return_weights=True)


def _run(name, dev, leaves=LEAVES, upstream=(0, 1, 2, 3), fn=_fused, samples=None, **kw):
    c, s = case_on(name, dev)
    s = samples or s
    dec = c["dec"]
    d = dict(planes=c["planes"].to(dev).requires_grad_("planes" in leaves), params=dec.mlp_params.to(dev).requires_grad_("params" in leaves),
             times=None if c["times"] is None else c["times"].to(dev),
             kw=dict(mask_out_of_bounds_samples=c["mask"], contract_coords=c["contract"],
                     scaffold=None if c["scaffold"] is None else c["scaffold"].to(dev)))
    d["dec"] = lp.DecoderParams(d["params"], dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
    rays = _rays(c, dev)
    rays.encoding.requires_grad_("enc" in leaves)
    out = fn(c, d, rays, s, **kw)
    if upstream and leaves:
        sum((out[i] * c["ups"][i].to(dev)).sum() for i in upstream if out[i] is not None).backward()
    return tuple(None if o is None else o.detach() for o in out), dict(planes=d["planes"].grad, params=d["params"].grad, enc=rays.encoding.grad)


@pytest.mark.parametrize("name", KC.ALL)
def test_values_and_gradients_against_fp64(name):
    dev = _dev()
    c, _ = case_on(name, dev)
    out, g = _run(name, dev)
    for key, a, b in zip(("ray_length", "neg_log_t", "feature", "weights"), out, c["out"]):
        _worst(f"{name} {key}", a, b)
    for k in LEAVES:
        _worst(f"{name} d {k}", g[k], c["grads"][k])
    assert not bool(g["planes"].cpu()[c["untouched"]].any()), "a row of the planes that no sample touches got a gradient"


@pytest.mark.parametrize("name", KC.ALL)
def test_against_the_chain_and_reproducible(name):
    dev = _dev()
    want, want_g = _run(name, dev, fn=_chain)
    got, got_g = _run(name, dev)
    assert torch.equal(got[3], want[3]), "weights differ from the chain's"
    for key, a, b in zip(("ray_length", "neg_log_t", "feature"), got, want):
        _worst(f"{name} {key} vs chain", a, b)
    for k in LEAVES:
        _worst(f"{name} d {k} vs chain", got_g[k], want_g[k])
    again, again_g = _run(name, dev)
    assert all(torch.equal(a, b) for a, b in zip(got, again)) and torch.equal(got_g["enc"], again_g["enc"])


@pytest.mark.parametrize("name", ["dynamic_222x32", "notrunk_022x32", "contract_mask_scaffold"])
def test_without_color(name):
    dev = _dev()
    c, _ = case_on(name, dev)
    want, _ = _run(name, dev)
    got, g = _run(name, dev, leaves=("planes", "params"), with_color=False)
    assert got[2] is None and all(torch.equal(got[i], want[i]) for i in (0, 1, 3))
    n_to = sum(i * o + o for v in (c["dec"].n_hidden_trunk, c["dec"].n_hidden_opacity)
               for dims in [lp.params.int_list_of(v)] for i, o in zip(dims[:-1], dims[1:]))
    assert not bool(g["params"][n_to:].any()) and bool(g["params"][:n_to].any()) and bool(g["planes"].any())


@pytest.mark.parametrize("leaves,upstream", [(("planes",), (0, 1, 2, 3)), (("params", "enc"), (0, 1, 2, 3)), (LEAVES, (3,))])
def test_subsets_of_leaves_and_upstreams(leaves, upstream):
    dev, name = _dev(), "dynamic_222x32"
    want_out, want = _run(name, dev)
    if upstream == (3,):   # the weights alone: the chain on the same upstream is the reference (no colour in the loss: d enc is 0)
        want = _run(name, dev, upstream=upstream, fn=_chain)[1]
    out, g = _run(name, dev, leaves, upstream)
    assert all(torch.equal(a, b) for a, b in zip(out, want_out))
    for k in LEAVES:
        if k in leaves:
            _worst(f"{leaves} {upstream} d {k}", g[k], want[k], tol=TOL if want[k].any() else 0.0)
        else:
            assert g[k] is None, k


def test_empty_batch():
    dev = _dev()
    c = KC.inputs("dynamic_222x32")
    rays = _rays(c, dev)
    rays = dataclasses.replace(rays, **{k: getattr(rays, k)[:0] for k in ("origins", "directions", "near", "far", "encoding", "grid_idx")})
    planes = c["planes"].to(dev).requires_grad_(True)
    z = torch.zeros(0, 65, device=dev)
    dec = dataclasses.replace(c["dec"], mlp_params=c["dec"].mlp_params.to(dev))
    out = lp.kplanes_render_samples(rays, torch.zeros(0, device=dev), z, z, planes, c["lay"], dec, return_weights=True)
    assert [tuple(o.shape) for o in out] == [(0,), (0,), (0, 3), (0, 65)]
    sum(o.sum() for o in out).backward()
    assert not bool(planes.grad.any())


def test_non_contiguous_depths():
    dev, name = _dev(), "dynamic_222x32"
    _, s = case_on(name, dev)
    wide = torch.zeros(9, 2 * 65 + 3, device=dev)
    wide[:, 1:131:2], wide[:, 2:132:2] = s.depths, s.deltas
    view = lp.RaySamples(s.points, wide[:, 1:131:2], wide[:, 2:132:2])
    assert not view.depths.is_contiguous()
    (want, want_g), (got, got_g) = _run(name, dev), _run(name, dev, samples=view)
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and torch.equal(got_g["enc"], want_g["enc"])


def _leaves_and_step(name, dev):
    c, s = case_on(name, dev)
    s = lp.RaySamples(s.points, s.depths.clone(), s.deltas.clone())
    planes, params = c["planes"].to(dev).requires_grad_(True), c["dec"].mlp_params.to(dev).requires_grad_(True)
    dec = lp.DecoderParams(params, c["dec"].n_hidden_trunk, c["dec"].n_hidden_opacity, c["dec"].n_hidden_color, c["dec"].color_chn)
    rays, times = _rays(c, dev), c["times"].to(dev)
    rays.encoding.requires_grad_(True)
    leaves, ups = [planes, params, rays.encoding], [u.to(dev) for u in c["ups"]]

    def step():
        for t in leaves:
            t.grad = None
        out = lp.kplanes_render_samples(rays, times, s.depths, s.deltas, planes, c["lay"], dec, gain=c["gain"], return_weights=True)
        torch.autograd.backward(out, ups)   # (no product tensors of the test's own)
        return out
    return c, s, leaves, step


def test_graph_capture_forward_and_backward():
    dev = _dev()
    c, s, leaves, step = _leaves_and_step("notrunk_022x32", dev)
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
    for round_ in range(3):
        with torch.no_grad():   # new values in the tensors the graph reads
            s.depths.mul_(0.95)
            leaves[0].mul_(1.1)
            leaves[2].add_(0.1)
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.detach().clone() for t in tuple(out) + tuple(captured)]
        eager = [t.detach() for t in tuple(step()) + tuple(t.grad for t in leaves)]
        for i, (a, b) in enumerate(zip(replayed, eager)):
            if i < 4 or i == 6:
                assert torch.equal(a, b), f"round {round_}: replayed tensor {i} != eager"
            else:
                _worst(f"round {round_}: replayed gradient {i} vs eager", a, b)


def test_memory_is_the_results_the_chunk_buffer_and_the_gradients():
    dev = _dev()
    c, s, leaves, step = _leaves_and_step("notrunk_022x32", dev)
    R, S = c["R"], c["S"]
    up512 = lambda n: (n + 511) // 512 * 512  # noqa: E731
    bound = sum(up512(4 * n) for n in (R, R, 3 * R, R * S, R * ((S + 63) // 64))) + sum(up512(4 * t.numel()) for t in leaves)
    for _ in range(2):   # (the first round loads the kernels)
        for t in leaves:
            t.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        out = step()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(dev) - before
        del out
    assert peak <= bound, (peak, bound)

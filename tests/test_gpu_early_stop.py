"""Early ray termination (``stop_transmittance``) against the TRUNCATED fp64 oracle, on the scripted batches of tests/early_stop_cases.py.

Per case, on every kernel family that has a DUMP twin:
* where each wavefront stopped -- the last marched sample the forward leaves in the closing checkpoint pair -- is uniform over the group
  and EQUAL to the index ``oracle.early_stop_index`` expects (no allowance: the host test proves that both decisive margins of every group
  are ten times what a kernel at the suite's bar can be off by);
* the flag words of the backward's dump say "contributed" exactly up to that index, "visited" exactly where a sibling wave of the
  workgroup marched further, and nothing behind;
* the proof (``forced_oracle_check``): the kernel's ReLU decisions AND its last samples are forced onto the fp64 oracle, every forced unit is
  a measured near tie, then all three outputs and every gradient family meet 1e-4 -- with non-zero upstream gradients on all three outputs,
  -log T included;
* the returned -log T is the truncated oracle's with the EXPECTED indices (nothing read back from the kernel);
* a ``torch.no_grad()`` forward is bit-identical to the grad-enabled one.
``LP_ARITH_FP32`` and the tuned family's eight-wave workgroups have no twin: test_gpu_parity.py::test_renderer_early_termination stays
what covers them."""
import ctypes

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib
from lightplane_amd.renderer import relu_dump_recorder
from tests import early_stop_cases as E
from tests.test_gpu_parity import (FORCED_EVENTS, REL_TOL, _assert_close, _dev, _rays_to, forced_oracle_check, has_dump_twin,
                                   run_hip_renderer)

pytestmark = pytest.mark.gpu


def _last_backward():
    fn = _lib.lib().lp_debug_last_renderer_backward
    fn.restype = ctypes.c_char_p
    return fn()


def _saved_ckpt(out):
    """neg_log_t_ckpt as the forward left it for the backward: saved tensor 1 of the LightplaneFunction node."""
    todo, seen = [out.grad_fn], set()
    while todo:
        node = todo.pop()
        if node is None or node in seen:
            continue
        seen.add(node)
        if type(node).__name__ == "LightplaneFunctionBackward":
            return node.saved_tensors[1].detach().cpu().clone()
        todo += [f for f, _ in node.next_functions]
    raise AssertionError("no LightplaneFunction node behind the output")


def _forward(d, dev, kernel, grad, **extra):
    rays = _rays_to(d["rays"], dev, grad)
    dec = d["decoder"]
    params = dec.mlp_params.to(dev).clone().requires_grad_(grad)
    hdec = lp.DecoderParams(params, dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
    grids = [g.to(dev).clone().requires_grad_(grad) for g in d["grids"]]
    cgrids = None if d["color_grids"] is None else [g.to(dev).clone().requires_grad_(grad) for g in d["color_grids"]]
    scaffold = None if d["scaffold"] is None else d["scaffold"].to(dev)
    with torch.set_grad_enabled(grad):
        out = lp.lightplane_renderer(rays, grids, hdec, scaffold=scaffold, color_grid=cgrids, kernel=kernel, **d["cfg"], **extra)
    ckpt = _saved_ckpt(out[1]) if grad else None
    return [o.detach().cpu() for o in out], ckpt


@pytest.mark.parametrize("case", E.CASES, ids=E.CASE_IDS)
def test_stop_indices_and_gradients_against_the_truncated_oracle(case):
    dev = _dev()
    d = E.build(case)
    eps, want = d["stop_transmittance"], d["last_sample"]
    assert all(float(u.abs().min()) > 0 for u in d["upstream"]), "the upstream gradient of an output is zero somewhere"
    assert has_dump_twin(d, kernel=case.kernel, stop_transmittance=eps), f"{case.name}: no DUMP twin"

    # ---- the forward: where it stopped ----
    out, ckpt = _forward(d, dev, case.kernel, True, stop_transmittance=eps)
    out_ng, _ = _forward(d, dev, case.kernel, False, stop_transmittance=eps)
    for nm, a, b in zip(("ray_length", "neg_log_t", "feature"), out, out_ng):
        assert torch.equal(a, b), f"{case.name}: {nm} of the torch.no_grad() forward differs from the grad-enabled one"
    s_last = ckpt.view(case.n_rays, -1, 2)[:, -1, 0]
    assert bool((s_last == s_last.round()).all())
    s_last = s_last.long()
    per_group = [s_last[lo:lo + case.group] for lo in range(0, case.n_rays, case.group)]
    print(f"{case.name}: last marched sample per group {[int(g[0]) for g in per_group]}, expected {d['expected'].index.tolist()}")
    for g, sl in enumerate(per_group):
        assert bool((sl == sl[0]).all()), f"{case.name}: group {g} holds several last samples: {sorted(set(sl.tolist()))}"
    assert torch.equal(s_last, want), (f"{case.name}: last marched samples per group {[int(g[0]) for g in per_group]}, the fp64 oracle expects "
                                       f"{d['expected'].index.tolist()}")
    # -log T as returned: the truncated oracle's, from the EXPECTED indices alone
    _assert_close(f"{case.name}: neg_log_t vs the truncated oracle", out[1], E.neg_log_t_cum(d, want)[:, -1].numpy())

    # ---- the backward: which samples it visited, which contributed ----
    with relu_dump_recorder() as rec:
        run_hip_renderer(d, dev, case.kernel, stop_transmittance=eps)
    if case.family == 1:
        # (random rays: the call asks for the transposed march, which has no vote -- with a stop the rays-per-wave kernels run)
        assert b"tuned family, rays per wavefront" in _last_backward(), _last_backward()
    flags = rec.dump[..., -1].cpu().long()
    expect = E.expected_flags(case, want)
    behind = (flags == 1) & (torch.arange(case.s_tot)[None, :] > want[:, None])
    assert not bool(behind.any()), f"{case.name}: {int(behind.sum())} samples behind their group's last one contributed to the backward"
    assert torch.equal(flags == 2, expect == 2), (f"{case.name}: visited-only samples at {int((flags == 2).sum())} places, expected "
                                                  f"{int((expect == 2).sum())}: exactly where a sibling wave marched further")
    assert torch.equal(flags, expect), f"{case.name}: {int((flags != expect).sum())} flag words differ from the expected map"

    # ---- the proof ----
    n0 = len(FORCED_EVENTS)
    forced_oracle_check(f"early-stop {case.name}", d, dev, kernel=case.kernel, stop_transmittance=eps)
    ev = FORCED_EVENTS[n0]
    assert ev["stopped_rays"] == int((want < case.s_tot - 1).sum()), "the proof truncated other rays than the expected ones"
    assert ev["visited_samples"] == int((expect != 0).sum())


def test_module_launch_with_background_and_alpha():
    """``LightplaneRenderer`` with ``bg_color`` and alpha under a stop (``config.stop_transmittance``): ``feature + T bg`` and ``1 - T`` of
    the truncated oracle, gradients included -- the backward's ``epilogue_grad_nlt`` with checkpoints behind the stop unwritten."""
    dev = _dev()
    case = E.CASES[0]
    d = E.build(case)
    bg = torch.tensor([0.2, 0.5, 0.9])
    dec = d["decoder"]
    mod = lp.LightplaneRenderer(num_samples=E.S, color_chn=3, grid_chn=case.grid_base[-1], mlp_hidden_chn=case.hidden, gain=case.gain,
                                bg_color=bg.tolist(), ray_embedding_num_harmonics=None).to(dev)
    assert mod.mlp_params.shape == dec.mlp_params.shape

    def runner(d, dev, kernel, **extra):
        assert kernel == _lib.LP_KERNEL_AUTO and not extra
        with torch.no_grad():
            mod.mlp_params.copy_(dec.mlp_params.to(dev))
        mod.mlp_params.grad = None
        rays = _rays_to(d["rays"], dev, True)
        grids = [g.to(dev).clone().requires_grad_(True) for g in d["grids"]]
        out = mod(rays, grids)
        torch.autograd.backward(list(out), [u.to(dev) for u in d["upstream"]])
        return out, mod.mlp_params.grad.clone(), rays.encoding.grad, [g.grad for g in grids], None

    def epilogue(o):
        t = torch.exp(-o[1])
        return o[0], 1 - t, o[2] + t[:, None] * bg.to(t.dtype)

    old = lp.config.stop_transmittance
    lp.config.stop_transmittance = d["stop_transmittance"]
    try:
        n0 = len(FORCED_EVENTS)
        _, prod, _ = forced_oracle_check(f"early-stop module {case.name}", d, dev, runner=runner, epilogue=epilogue, return_results=True)
    finally:
        lp.config.stop_transmittance = old
    assert FORCED_EVENTS[n0]["stopped_rays"] == int((d["last_sample"] < case.s_tot - 1).sum())
    # alpha and the composited feature, from the expected indices alone
    nlt = E.neg_log_t_cum(d, d["last_sample"])[:, -1]
    _assert_close("module alpha vs the truncated oracle", prod[0][1], (1 - torch.exp(-nlt)).numpy(), tol=REL_TOL)

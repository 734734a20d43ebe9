"""Worker of tests/test_gpu_deep_forward.py: early termination (stop_transmittance) on a dense scene through the workgroup-synchronous
forward of the deep hidden-64 decoders.  The one failure a desynchronised barrier of that kernel would produce is a hang, so the launch
runs in this process of its own and the test waits for it under a time limit.

    python tests/deep_forward_stop_worker.py T,O,C SEED FAMILY     -> "DEEP_STOP_OK" and exit status 0

556 rays = two full workgroups of 256 and one of 44 (one full wave, one of 12 rays, six waves without a ray):
  workgroup 0: [64 fastest-saturating rays][64 slowest-saturating rays][64 rays that never saturate][32 saturating + 32 that never do]
               -- two wavefronts that stop, at different samples, next to one that marches to the end and a mixed one;
  workgroup 1: 256 saturating rays, ordered by density -- every wave stops, the workgroup leaves the sample loop early and together;
  workgroup 2: 44 saturating rays -- the same exit, taken with waves that never held a ray.

The same launch is then PROVEN against the truncated fp64 oracle (tests/test_gpu_parity.py ``forced_oracle_check``, with a non-zero
upstream gradient on -log T as well): the backward's own ReLU decisions and last marched samples forced onto the oracle, every output and
gradient at 1e-4; and every 64-ray group's last sample is the one ``oracle.early_stop_index`` expects wherever the oracle's two decisive
margins clear the tie bar of tests/early_stop_cases.py (the rays are picked by the kernels here, not solved for margins).
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch

import lightplane_amd as lp
from lightplane_amd import _lib
from oracle import lightplane_oracle as O
from tests import early_stop_cases as E
from tests.synth import RendererCase
from tests.test_gpu_parity import FORCED_EVENTS, _rays_to, forced_oracle_check, has_dump_twin

EPS = 1e-5
N_RAYS = 556


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


def _run(d, dev, kernel, backward=True, **extra):
    """tests.test_gpu_parity.run_hip_renderer, which also hands back the checkpoints the forward saved."""
    rays = _rays_to(d["rays"], dev, True)
    dec = d["decoder"]
    params = dec.mlp_params.to(dev).clone().requires_grad_(True)
    hdec = lp.DecoderParams(params, dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
    grids = [g.to(dev).clone().requires_grad_(True) for g in d["grids"]]
    scaffold = d["scaffold"].to(dev)
    out = lp.lightplane_renderer(rays, grids, hdec, scaffold=scaffold, kernel=kernel, **d["cfg"], **extra)
    ckpt = _saved_ckpt(out[1])
    if not backward:
        return [o.detach().cpu() for o in out[:3]], ckpt, None
    g_len, g_nlt, g_feat = (t.to(dev) for t in d["upstream"])
    ((out[0] * g_len).sum() + (out[1] * g_nlt).sum() + (out[2] * g_feat).sum()).backward()
    torch.cuda.synchronize()
    grads = [("params", params.grad.cpu()), ("enc", rays.encoding.grad.cpu())] + [(f"grid{i}", g.grad.cpu()) for i, g in enumerate(grids)]
    return [o.detach().cpu() for o in out[:3]], ckpt, grads


def main(layers, seed, family):
    dev = torch.device("cuda:0")
    lp.config.deep_forward_mfma = True
    lp.config.warn_generic_kernel = False
    S = 40
    # a dense scene (gain x 40) whose x < 0 half is empty space (scaffold occupancy 0), 8 000 random rays; the exact march says which
    # rays saturate and how fast
    d = RendererCase("deep_stop", seed=seed, n_rays=8000, grid_base=(1, 8, 8, 8, 32), n_layers=layers, hidden=64, num_samples=S, gain=40.0).build()
    d["scaffold"] = torch.ones(1, 4, 4, 4)
    d["scaffold"][..., :2] = 0.0
    assert lp.forward_kernel_family(d["rays"], d["grids"], d["decoder"]) == family
    nlt = _run(d, dev, _lib.LP_KERNEL_AUTO, backward=False)[0][1]
    dense = torch.nonzero(nlt > 4 * -np.log(EPS)).flatten()[:1000]
    empty = torch.nonzero(nlt < 0.5 * -np.log(EPS)).flatten()
    # the sample at which each dense ray ALONE is through: 64 copies of it fill one wavefront of the shape-generic forward, whose
    # closing checkpoint pair holds the last sample that wavefront marched
    full = d["rays"]
    d["rays"] = full[dense.repeat_interleave(64)]
    stop = _run(d, dev, _lib.LP_KERNEL_GENERIC, backward=False, stop_transmittance=EPS)[1][::64, -2]
    d["rays"] = full
    early = stop <= S - 4
    dense, stop = dense[early], stop[early]
    order = torch.argsort(stop)
    dense, stop = dense[order], stop[order]  # first through first
    assert len(dense) >= 460 and len(empty) >= 96, (len(dense), len(empty))
    assert float(stop[63]) < float(stop[-1]), "the scene has no rays that saturate at different samples"
    fast, slow, mid = dense[:64], dense[-64:], dense[64:-64]
    mid = mid[::max(1, len(mid) // 332)]
    idx = torch.cat([fast, slow, empty[:64], mid[:32], empty[64:96], mid[32:288], mid[288:332]])
    assert len(idx) == N_RAYS and len(torch.unique(idx)) == N_RAYS
    d["rays"] = d["rays"][idx]
    g_len, g_nlt, g_feat = d["upstream"]
    up_all = (g_len[idx], g_nlt[idx], g_feat[idx])
    d["upstream"] = (g_len[idx], torch.zeros_like(g_nlt[idx]), g_feat[idx])  # no loss on -log T

    out0, _, gr0 = _run(d, dev, _lib.LP_KERNEL_AUTO)
    out1, ck1, gr1 = _run(d, dev, _lib.LP_KERNEL_AUTO, stop_transmittance=EPS)
    _, ckg, _ = _run(d, dev, _lib.LP_KERNEL_GENERIC, backward=False, stop_transmittance=EPS)
    nlt0, nlt1 = out0[1], out1[1]
    stopped = nlt1 < nlt0 * (1 - 1e-6) - 1e-6
    s_last = ck1[:, -2]   # the closing checkpoint pair: (last marched sample, low word of -log T)
    print(f"{layers}: {int(stopped.sum())} of {N_RAYS} rays stopped early; last marched sample per 64-ray wavefront: "
          f"{[int(s_last[w]) for w in range(0, N_RAYS, 64)]}", flush=True)
    # the termination rule is the generic forward's: the same last marched sample for every ray
    assert torch.equal(s_last, ckg[:, -2]), "the last marched samples differ from the shape-generic forward's"
    for w in range(0, N_RAYS, 64):
        assert bool((s_last[w:w + 64] == s_last[w]).all()), f"rays {w}..: one wavefront, several last samples"
    # workgroup 0: two wavefronts stop, at different samples, one never stops, one is mixed and marches on
    assert bool(stopped[0:64].any()) and bool(stopped[64:128].any()), "workgroup 0: no early stop"
    assert int(s_last[0]) < int(s_last[64]) < S - 1, "workgroup 0: the two stopping wavefronts did not stop at different samples"
    assert not bool(stopped[128:256].any()) and int(s_last[128]) == S - 1 and int(s_last[192]) == S - 1
    # workgroups 1 and 2: every wavefront stops, the workgroup leaves before the last sample; not all at one sample
    assert bool((s_last[256:] < S - 1).all()), "the all-dense workgroups marched to the end"
    assert len(set(int(s_last[w]) for w in range(256, 512, 64))) > 1, "workgroup 1: every wavefront stopped at the same sample"
    # the bar of tests/test_gpu_parity.py::test_renderer_early_termination
    assert bool((nlt1[stopped] >= -np.log(EPS) - 1e-4).all())
    assert bool((nlt1 <= nlt0 * (1 + 1e-6) + 1e-6).all())
    far = float(d["rays"].far.max())
    assert float((out1[0] - out0[0]).abs().max()) <= 2 * EPS * far * 4
    assert float((out1[2] - out0[2]).abs().max()) <= 2 * EPS * 4
    for (nm, a), (_, b) in zip(gr1, gr0):
        scale = float(b.abs().max()) + 1e-30
        assert float((a - b).abs().max()) / scale <= 1e-3, nm

    # the proof: this forward, the shape-generic backward (64-ray groups), against the truncated fp64 oracle
    d["upstream"] = up_all
    assert has_dump_twin(d, stop_transmittance=EPS)
    forced_oracle_check(f"early-stop deep forward {layers}", d, dev, stop_transmittance=EPS)
    s_last = s_last.long()
    assert FORCED_EVENTS[-1]["stopped_rays"] == int((s_last < S - 1).sum()), "the backward contributed other samples than the forward marched"
    nlt = E.neg_log_t_cum(d)
    want = O.early_stop_index(nlt, -np.log(EPS), 64)
    returned = nlt.gather(1, s_last[:, None])[:, 0]
    bar = E.TIE_FACTOR * E.OUTPUT_BAR * float(returned.max())
    decided = (want.margin_reached >= bar) & (want.margin_before >= bar)
    got = s_last[::64]
    print(f"{layers}: oracle's last samples {want.index.tolist()}, margins reached {[round(float(v), 3) for v in want.margin_reached]} / before "
          f"{[round(float(v), 3) for v in want.margin_before]}, tie bar {bar:.4f}: {int(decided.sum())} of {len(got)} groups decided", flush=True)
    # (the two groups of workgroup 0 that never stop are decided by construction: the comparison has to reach groups that do stop)
    assert int((decided & (want.index < S - 1)).sum()) >= 3, "the oracle's margins decide too few stopping groups for the comparison to mean anything"
    assert torch.equal(got[decided], want.index[decided]), (got.tolist(), want.index.tolist())
    print("DEEP_STOP_OK", flush=True)


if __name__ == "__main__":
    main(tuple(int(v) for v in sys.argv[1].split(",")), int(sys.argv[2]), int(sys.argv[3]))

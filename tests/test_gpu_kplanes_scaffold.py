"""The fused scaffold of a plane field (lp_kplanes_scaffold.hip) against the fp64 reference of tests/kplanes_scaffold_cases.py: the
opacity lattice within the project's bar, the occupancy exactly, at thresholds whose gap tests/test_kplanes_scaffold_host.py holds."""
import pytest
import torch

import lightplane_amd as lp
from tests import kplanes_scaffold_cases as SC
from tests.test_gpu_parity import _dev, _rel_err
from tests.test_gpu_ray_grid import _warm_up
from tests.test_gpu_scaffold import oracle_occupancy

pytestmark = pytest.mark.gpu
BAR = 1e-4   # max |err| / max |ref|: the project's bar


def _opacity(c, dev, times="case", **kw):
    planes, dec, t = SC.on_device(c, dev)
    return lp.kplanes_scaffold_opacity(planes, c["lay"], dec, c["size"], times=t if isinstance(times, str) else times, gain=SC.GAIN, **kw)


def _occupancy(c, dev, threshold, r, **kw):
    planes, dec, t = SC.on_device(c, dev)
    return lp.kplanes_calculate_scaffold(planes, c["lay"], dec, c["size"], times=t, gain=SC.GAIN, threshold=threshold, dilate_scaffold=r,
                                         **kw)


@pytest.mark.parametrize("name", SC.ALL)
def test_opacity_lattice(name):
    dev, c = _dev(), SC.case(name)
    got = _opacity(c, dev)
    assert got.shape == tuple(c["size"]) and got.dtype == torch.float32 and got.device == dev
    worst = _rel_err(got, c["op"].numpy())
    print(f"{name}: worst |err| / max |ref| = {worst:.3e}")
    assert worst <= BAR
    assert torch.equal(_opacity(c, dev), got)   # bit-reproducible
    if c["times"] is not None:                  # the maximum does not depend on the order of the timestamps
        assert torch.equal(_opacity(c, dev, times=c["times"].flip(0).to(dev)), got)


@pytest.mark.parametrize("name", SC.ALL)
def test_occupancy_is_exact(name):
    dev, c = _dev(), SC.case(name)
    got = _occupancy(c, dev, c["t"], c["r"])
    assert got.shape == tuple(c["size"]) and got.dtype == torch.float32
    bad = int((got.cpu() != oracle_occupancy(c["op"], c["t"], c["r"])).sum())
    assert bad == 0, f"{name}, dilate {c['r']}: {bad} of {got.numel()} lattice points differ from the oracle"
    # without dilation it is the thresholded opacity lattice: the early exit of the time loop changes nothing
    assert torch.equal(_occupancy(c, dev, c["t"], 0), (_opacity(c, dev) > c["t"]).float())
    out = torch.full(c["size"], 7.0, device=dev)
    ws = torch.empty(lp.kplanes_scaffold_workspace_bytes(c["size"], c["r"]) + 3, dtype=torch.uint8, device=dev)
    assert _occupancy(c, dev, c["t"], c["r"], out=out, workspace=ws) is out and torch.equal(out, got)


@pytest.mark.parametrize("name", ["dyn_22x32_w70", "static_11x32"])
def test_thresholds_below_and_above_every_value(name):
    dev, c = _dev(), SC.case(name)
    lo, hi = 0.5 * float(c["op"].min()), 2.0 * float(c["op"].max())
    for r in (0, c["r"] + 1):
        assert float(_occupancy(c, dev, lo, r).min()) == 1.0 and float(_occupancy(c, dev, hi, r).max()) == 0.0


def test_graph_capture():
    """captured once, replayed on new planes and timestamps written in place: the replays are the eager results"""
    dev, c = _dev(), SC.case("dyn_22x32_w70")
    planes, dec, times = SC.on_device(c, dev)
    out = torch.empty(c["size"], device=dev)
    ws = torch.empty(lp.kplanes_scaffold_workspace_bytes(c["size"], c["r"]), dtype=torch.uint8, device=dev)
    kw = dict(times=times, gain=SC.GAIN, threshold=c["t"], dilate_scaffold=c["r"])
    run = lambda **o: lp.kplanes_calculate_scaffold(planes, c["lay"], dec, c["size"], **kw, **o)  # noqa: E731
    _warm_up(lambda: run(out=out, workspace=ws))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(out=out, workspace=ws)
    for round_ in range(3):
        if round_ > 0:   # new values in the tensors the graph reads
            planes.copy_(planes.roll(round_, 1).flip(2))
            times.copy_(torch.tensor([0.9, -0.2, 0.1]) * round_)
        out.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        eager = run()
        assert torch.equal(out, eager) and 0 < float(eager.mean()) < 1, round_
    assert not torch.equal(out.cpu(), oracle_occupancy(c["op"], c["t"], c["r"]))   # (the new inputs give another scaffold)

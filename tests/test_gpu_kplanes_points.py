"""The decoder on a plane field at points in one launch (lightplane_amd/kplanes.py ``kplanes_eval_mlp``, csrc/lp_kplanes_points.hip)
against the fp64 reference of tests/kplanes_points_cases.py: every tensor to max |err| / max |ref| <= 1e-4, re-ordered atomic sums
against the all-leaves run at BAR_ATOMIC; the worst value is printed before it is held.  Measured worst errors: DESIGN.md 4.26."""
import pytest
import torch

from tests import kplanes_points_cases as KC
from tests.test_gpu_parity import _dev
from tests.test_gpu_ray_grid import BAR_ATOMIC, _warm_up, _worst

pytestmark = pytest.mark.gpu

LEAVES = ("points", "planes", "params", "enc")


def _backward(c, d, dev, op, col):
    loss = (op * c["u_op"].to(dev)).sum()
    return (loss if col is None else loss + (col * c["u_col"].to(dev)).sum()).backward()


@pytest.mark.parametrize("name", KC.ALL)
def test_values(name):
    dev, c = _dev(), KC.case(name)
    d = KC.on_device(c, dev)
    op, col = KC.evaluate(c, d)
    assert op.shape == c["op"].shape and col.shape == c["col"].shape and op.dtype == col.dtype == torch.float32
    _worst(f"{name} opacity", op, c["op"], ~c["left_out"])
    _worst(f"{name} colour", col, c["col"], ~c["left_out"])
    op2, col2 = KC.evaluate(c, d)
    assert torch.equal(op2, op) and torch.equal(col2, col), "a second forward differs (it has no atomics)"
    assert torch.equal(KC.evaluate(c, d, opacity_only=True), op), "opacity-only differs from the joint opacity"
    empty = ((c["occ"] == 0) & ~c["left_out"]).to(dev)
    assert float(op[empty].abs().sum()) == 0.0 and float(col[empty].abs().sum()) == 0.0, "occ = 0, but a result is not exactly 0"


@pytest.mark.parametrize("name", KC.ALL)
def test_gradients(name):
    dev, c = _dev(), KC.case(name)
    d = KC.on_device(c, dev, LEAVES)
    _backward(c, d, dev, *KC.evaluate(c, d))
    for k in LEAVES:
        _worst(f"{name} d {k}", d[k].grad, c["grads"][k])
    assert float(d["planes"].grad.cpu()[c["untouched"]].abs().sum()) == 0.0, "a row no point touches is not exactly 0"
    again = KC.on_device(c, dev, ("points",))
    _backward(c, again, dev, *KC.evaluate(c, again))
    assert torch.equal(again["points"].grad, d["points"].grad), "a second point gradient differs"
    # the masked points alone: exactly nothing for the planes and the points
    gone = (~c["inside"] & ~c["left_out"]).to(dev)
    m = KC.on_device(c, dev, ("points", "planes"))
    op, col = KC.evaluate(c, m)
    ((op * gone).sum() + (col * gone[..., None]).sum()).backward()
    assert float(m["planes"].grad.abs().sum()) == 0.0 and float(m["points"].grad[gone].abs().sum()) == 0.0, "a masked point has a gradient"
    # without a colour gradient the colour MLP gets exactly 0
    o = KC.on_device(c, dev, ("params",))
    (KC.evaluate(c, o)[0] * c["u_op"].to(dev)).sum().backward()
    dims = [int(v) for v in c["dec"].n_hidden_color]
    n_color = sum(i * w + w for i, w in zip(dims[:-1], dims[1:]))
    assert float(o["params"].grad[-n_color:].abs().sum()) == 0.0 and float(o["params"].grad[:-n_color].abs().sum()) > 0.0


@pytest.mark.parametrize("name", ["dynamic_222x32", "contract_mask_scaffold"])
@pytest.mark.parametrize("asked", [("planes",), ("params",), ("points", "enc")])
def test_only_some_gradients(name, asked):
    dev, c = _dev(), KC.case(name)
    full, part = KC.on_device(c, dev, LEAVES), KC.on_device(c, dev, asked)
    _backward(c, full, dev, *KC.evaluate(c, full))
    _backward(c, part, dev, *KC.evaluate(c, part))
    for k in LEAVES:
        if k not in asked:
            assert part[k].grad is None, f"{k} got a gradient nobody asked for"
        elif k == "points":
            assert torch.equal(part[k].grad, full[k].grad), "the point gradient depends on who else asks"
        else:
            _worst(f"{name}: d {k} with {asked} vs all leaves", part[k].grad, full[k].grad, tol=BAR_ATOMIC)


@pytest.mark.parametrize("shape", [(0, 5), (3, 0)])
def test_empty_batch(shape):
    dev, c = _dev(), KC.case("dynamic_222x32")
    d = KC.on_device(c, dev, ("planes", "params"))
    pts = torch.zeros(shape + (3,), device=dev, requires_grad=True)
    enc = torch.zeros(shape[0], d["enc"].shape[1], device=dev, requires_grad=True)
    op, col = KC.evaluate(c, d, points=pts, enc=enc, times=torch.zeros(shape[0], device=dev),
                          gidx=torch.zeros(shape[0], dtype=torch.int64, device=dev))
    assert op.shape == shape and col.shape == shape + (3,)
    (op.sum() + col.sum()).backward()
    for t in (d["planes"], d["params"], pts, enc):
        assert t.grad.shape == t.shape and float(t.grad.abs().sum()) == 0.0


def test_graph_capture_forward_and_backward():
    """captured once, replayed on new values: values and the point gradient to the bit, the atomically summed gradients to BAR_ATOMIC"""
    dev, c = _dev(), KC.case("dynamic_222x32")
    d, static = KC.on_device(c, dev, LEAVES), {}
    c = dict(c, gidx=c["gidx"].to(dev), u_op=c["u_op"].to(dev), u_col=c["u_col"].to(dev))   # (no copy to the device inside the capture)

    def step():
        for k in LEAVES:
            d[k].grad = None
        op, col = KC.evaluate(c, d)
        _backward(c, d, dev, op, col)
        static.update(op=op.detach(), col=col.detach(), **{k: d[k].grad for k in LEAVES})

    _warm_up(step)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    captured = dict(static)
    gen = torch.Generator().manual_seed(83)
    for round_ in range(3):
        if round_:  # new values in the tensors the graph reads
            with torch.no_grad():
                d["planes"].copy_(0.5 + torch.rand(d["planes"].shape, generator=gen))
                d["points"].copy_((torch.rand(d["points"].shape, generator=gen) * 2 - 1) * 1.2)
        graph.replay()
        torch.cuda.synchronize()
        replayed = {k: v.clone() for k, v in captured.items()}
        step()
        for k in ("op", "col", "points"):
            assert torch.equal(replayed[k], static[k]), f"round {round_}: replayed {k} != eager"
        for k in ("planes", "params", "enc"):
            _worst(f"round {round_}: replayed d {k} vs eager", replayed[k], static[k], tol=BAR_ATOMIC)
    assert float((static["op"].cpu().double() - c["op"]).abs().max()) > 1e-3  # (the later rounds really saw other values)

"""The fused decoder evaluation at points (lightplane_amd/points.py, csrc/lp_points.hip) against its fp64 definition.

Oracle, inputs, and the points left out / zeroed: tests/points_cases.py (its docstring states every condition and cap;
tests/test_points_host.py::test_inputs_are_admissible checks them without a GPU).  Every comparison is held to the project's bar,
max |err| / max |ref| <= 1e-4, and prints its figure before it asserts.
"""
import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import config
from oracle import lightplane_oracle as O
from tests import points_cases as PC
from tests.synth import grid_sizes_for
from tests.test_gpu_parity import _assert_close, _dev

pytestmark = pytest.mark.gpu


def _joint(d, c):
    return lp.lightplane_eval_mlp(d["pts"], d["grid"], d["gidx"], d["dec"], d["enc"], PC.GAIN, c["mask"], None, d["scaffold"],
                                  d["color_grid"], c["contract"], grid_sizes=d["sizes"], color_grid_sizes=d["color_sizes"])


def _opacity_only(d, c):
    return lp.lightplane_eval_mlp_opacity_only(d["pts"], d["grid"], d["gidx"], d["dec"], PC.GAIN, c["mask"], None, d["scaffold"],
                                               c["contract"], grid_sizes=d["sizes"])


def _worst(name, got, want, keep=None):
    """max |err| / max |ref| over the kept entries, printed and held to the bar"""
    got, want = got.detach().double().cpu(), want.double()
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    if keep is not None:
        k = keep.reshape(keep.shape + (1,) * (want.ndim - keep.ndim)).expand_as(want)
        got, want = got[k], want[k]
    scale = max(float(want.abs().max()), 1e-30)
    err = float((got - want).abs().max()) / scale
    print(f"{name}: max |err| / max |ref| = {err:.3e} (max |ref| {scale:.4g})")
    assert err <= PC.TOL, f"{name}: {err:.3e} > {PC.TOL}"


@pytest.mark.parametrize("name", list(PC.CASES))
def test_values(name):
    dev, c = _dev(), PC.case(name)
    d = PC.on_device(c, dev)
    op, col = _joint(d, c)
    R, N = c["pts"].shape[:2]
    assert op.shape == (R, N) and col.shape == (R, N, 3) and op.dtype == col.dtype == torch.float32 and op.device == dev
    keep = ~c["left_out"]
    assert int(c["left_out"].sum()) <= PC.MAX_LEFT_OUT * keep.numel()
    _worst(f"{name} opacity", op, c["op"], keep)
    _worst(f"{name} colour", col, c["col"], keep)
    assert torch.equal(_opacity_only(d, c), op), "the opacity-only call and the joint call's opacity differ"
    if c["scaffold"] is not None:  # a removed point is exactly zero in both results
        gone = (c["op"] == 0) & keep
        assert int(gone.sum()) > 0 and float(op.cpu()[gone].abs().max()) == 0.0 and float(col.cpu()[gone].abs().max()) == 0.0


@pytest.mark.parametrize("name", list(PC.CASES))
def test_gradients(name):
    dev, c = _dev(), PC.case(name)
    n = c["zeroed"].numel()
    assert int(c["zeroed"].sum()) <= PC.MAX_ZEROED * n or n == 1 and not bool(c["zeroed"].any())
    d = PC.on_device(c, dev, requires_grad=("points", "params", "enc", "grids", "cgrids"))
    op, col = _joint(d, c)
    ((op * c["u_op"].to(dev)).sum() + (col * c["u_col"].to(dev)).sum()).backward()
    gr = c["grads"]
    as_list = lambda g: g if isinstance(g, list) else [g]  # noqa: E731
    for i, (t, want) in enumerate(zip(as_list(d["grid"]), PC.flat_grad(c, gr["grids"]))):
        _worst(f"{name} d grid[{i}]", t.grad, want)
    if c["cgrids"] is not None:
        for i, (t, want) in enumerate(zip(as_list(d["color_grid"]), PC.flat_grad(c, gr["cgrids"]))):
            _worst(f"{name} d color_grid[{i}]", t.grad, want)
    _worst(f"{name} d mlp_params", d["params"].grad, gr["params"])
    _worst(f"{name} d rays_encoding", d["enc"].grad, gr["enc"])
    _worst(f"{name} d points", d["pts"].grad, gr["points"])


def test_opacity_only_gives_exactly_zero_colour_parameter_gradient():
    dev, c = _dev(), PC.case("triplane_c16_222x32")
    d = PC.on_device(c, dev, requires_grad=("params", "grids"))
    op = _opacity_only(d, c)
    (op * c["u_op"].to(dev)).sum().backward()
    dec = c["dec"]
    n_color = lp.params.mlp_numel(dec.n_hidden_color)
    g = d["params"].grad
    assert float(g[-n_color:].abs().max()) == 0.0 and float(g[:-n_color].abs().max()) > 0.0
    # the joint call differentiated through its opacity alone: the colour head is not evaluated either -- the same gradients, bit for
    # bit in the parameters' colour part, to the bar elsewhere (atomics: the summation order differs from call to call)
    d2 = PC.on_device(c, dev, requires_grad=("params", "grids", "enc"))
    op2, _ = _joint(d2, c)
    (op2 * c["u_op"].to(dev)).sum().backward()
    assert float(d2["params"].grad[-n_color:].abs().max()) == 0.0 and float(d2["enc"].grad.abs().max()) == 0.0
    _worst("opacity-only vs joint, d mlp_params", d2["params"].grad, g.cpu())
    for a, b in zip(d2["grid"], d["grid"]):
        _worst("opacity-only vs joint, d grid", a.grad, b.grad.cpu())


@pytest.mark.parametrize("subset", [("points",), ("params",), ("enc",), ("grids",), ("cgrids", "points")])
def test_gradients_follow_requires_grad(subset):
    dev, c = _dev(), PC.case("voxel_c32_twogrid_022x32")
    d = PC.on_device(c, dev, requires_grad=subset)
    op, col = _joint(d, c)
    ((op * c["u_op"].to(dev)).sum() + (col * c["u_col"].to(dev)).sum()).backward()
    gr = c["grads"]
    leaves = {"points": [d["pts"]], "params": [d["params"]], "enc": [d["enc"]], "grids": d["grid"], "cgrids": d["color_grid"]}
    wants = {"points": [gr["points"]], "params": [gr["params"]], "enc": [gr["enc"]], "grids": gr["grids"], "cgrids": gr["cgrids"]}
    for key, ts in leaves.items():
        for t, want in zip(ts, wants[key]):
            if key in subset:
                _worst(f"requires_grad {subset}: d {key}", t.grad, want)
            else:
                assert t.grad is None, f"{key} does not require a gradient and got one"


def test_empty_batches():
    dev, c = _dev(), PC.case("triplane_c16_222x32")
    d = PC.on_device(c, dev, requires_grad=("params",))
    for shape in ((0, 5), (4, 0)):
        pts = torch.zeros(*shape, 3, device=dev)
        idx, enc = torch.zeros(shape[0], dtype=torch.long, device=dev), torch.zeros(shape[0], 32, device=dev)
        op, col = lp.lightplane_eval_mlp(pts, d["grid"], idx, d["dec"], enc, PC.GAIN)
        assert op.shape == shape and col.shape == shape + (3,)
        (op.sum() + col.sum()).backward()
        assert float(d["params"].grad.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------------------
# module
# ------------------------------------------------------------------------------------------------------------------------------

def _module_inputs(dev, two_grid=False):
    """the inputs of tests/test_gpu_parity.py::test_module_point_evaluation_and_scaffold"""
    torch.manual_seed(0)
    mod = lp.LightplaneRenderer(num_samples=8, color_chn=3, grid_chn=16, mlp_hidden_chn=32, gain=2.0, opacity_init_bias=-1.0,
                                ray_embedding_num_harmonics=None, use_separate_color_grid=two_grid).to(dev)
    with torch.no_grad():
        mod.mlp_params.mul_(3.0)
    grids = [0.5 * torch.randn(s) for s in grid_sizes_for((2, 6, 5, 7, 16), True)]
    pts = torch.rand(5, 11, 3) * 2.4 - 1.2
    gidx = torch.tensor([0, 1, 1, 0, 1])
    enc = torch.randn(5, mod.rays_encoding_dim)
    cgrids = [0.5 * torch.randn(g.shape) for g in grids] if two_grid else None
    return mod, grids, cgrids, pts, gidx, enc


@pytest.mark.parametrize("two_grid", [False, True])
def test_module_calls_the_fused_functions(two_grid):
    dev = _dev()
    mod, grids, cgrids, pts, gidx, enc = _module_inputs(dev, two_grid)
    dg = [g.to(dev) for g in grids]
    dc = None if cgrids is None else [g.to(dev) for g in cgrids]
    dpts, didx, denc = pts.to(dev), gidx.to(dev), enc.to(dev)
    dec = mod.get_decoder_params()
    cdec = lp.DecoderParams(dec.mlp_params.detach().cpu(), dec.n_hidden_trunk.cpu(), dec.n_hidden_opacity.cpu(), dec.n_hidden_color.cpu(), 3)
    assert config.fused_module_ops
    for mask in (False, True):
        with torch.no_grad():
            op = mod.eval_opacity_at_points(dpts, didx, dg, mask_out_of_bounds_samples=mask)
            op2, col = mod.eval_decoder_at_points(dpts, didx, denc, dg, dc, mask_out_of_bounds_samples=mask)
            f_op = lp.lightplane_eval_mlp_opacity_only(dpts, dg, didx, dec, 2.0, mask)
            f_op2, f_col = lp.lightplane_eval_mlp(dpts, dg, didx, dec, denc, 2.0, mask, color_grid=dc)
            assert torch.equal(op, f_op) and torch.equal(op2, f_op2) and torch.equal(col, f_col) and torch.equal(op, op2)
            config.fused_module_ops = False
            try:
                r_op = mod.eval_opacity_at_points(dpts, didx, dg, mask_out_of_bounds_samples=mask)
                r_op2, r_col = mod.eval_decoder_at_points(dpts, didx, denc, dg, dc, mask_out_of_bounds_samples=mask)
            finally:
                config.fused_module_ops = True
        assert not torch.equal(r_op, op) or not torch.equal(r_col, col)  # (another kernel: the switch really switches)
        _assert_close("opacity, fused vs Renderer path", op, r_op.cpu().numpy(), tol=2e-5)
        _assert_close("opacity (joint), fused vs Renderer path", op2, r_op2.cpu().numpy(), tol=2e-5)
        _assert_close("colour, fused vs Renderer path", col, r_col.cpu().numpy(), tol=2e-5)
        o_op, o_col = O.eval_decoder(pts, grids, gidx, cdec, enc, 2.0, mask_out_of_bounds_samples=mask, color_grids=cgrids)
        _assert_close("opacity vs oracle", op, o_op.numpy(), tol=2e-5)
        _assert_close("colour vs oracle", col, o_col[..., :3].numpy(), tol=2e-5)
    # the flat form, which the Renderer path of eval_decoder_at_points never took
    flat = torch.cat([g.reshape(-1, 16) for g in dg])
    sizes = [list(g.shape) for g in grids]
    cflat = None if dc is None else torch.cat([g.reshape(-1, 16) for g in dc])
    with torch.no_grad():
        a_op, a_col = mod.eval_decoder_at_points(dpts, didx, denc, dg, dc)
        b_op, b_col = mod.eval_decoder_at_points(dpts, didx, denc, flat, cflat, grid_sizes=sizes, color_grid_sizes=None if dc is None else sizes)
    assert torch.equal(a_op, b_op) and torch.equal(a_col, b_col)


def test_module_backpropagates_opacity_and_colour_in_one_call():
    dev = _dev()
    mod, grids, _, pts, gidx, enc = _module_inputs(dev)
    dg = [g.to(dev).requires_grad_(True) for g in grids]
    op, col = mod.eval_decoder_at_points(pts.to(dev), gidx.to(dev), enc.to(dev), dg)
    (op.sum() + col.sum()).backward()
    dec = mod.get_decoder_params()
    g64 = [g.double().requires_grad_(True) for g in grids]
    p64 = dec.mlp_params.detach().cpu().double().requires_grad_(True)
    cdec = lp.DecoderParams(p64, dec.n_hidden_trunk.cpu(), dec.n_hidden_opacity.cpu(), dec.n_hidden_color.cpu(), 3)
    o_op, o_col = O.eval_decoder(pts.double(), g64, gidx, cdec, enc.double(), 2.0)
    (o_op.sum() + o_col[..., :3].sum()).backward()
    _worst("module d mlp_params", mod.mlp_params.grad, p64.grad)
    for i, (g, w) in enumerate(zip(dg, g64)):
        _worst(f"module d grid[{i}]", g.grad, w.grad)


# ------------------------------------------------------------------------------------------------------------------------------
# graph capture, memory
# ------------------------------------------------------------------------------------------------------------------------------

def _warm_up(fn, times=1):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(times):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


def test_graph_capture_forward_and_backward():
    """the forward alone and the forward + backward chain, each captured once and replayed on new grid values: every replay equals the
    eager result on the same values (results and the stored point gradient to the bit; gradients summed with atomics to the bar)"""
    dev, c = _dev(), PC.case("triplane_c16_222x32")
    d = PC.on_device(c, dev, requires_grad=("params", "grids", "enc", "points"))
    u_op, u_col = c["u_op"].to(dev), c["u_col"].to(dev)
    leaves = list(d["grid"]) + [d["params"], d["enc"], d["pts"]]

    def clear():
        for t in leaves:
            t.grad = None

    def forward():
        with torch.no_grad():
            return _joint(d, c)

    def step():
        clear()
        op, col = _joint(d, c)
        ((op * u_op).sum() + (col * u_col).sum()).backward()

    _warm_up(forward)
    g_fwd = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_fwd):
        out = forward()
    _warm_up(step, 3)
    clear()
    g_bwd = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_bwd):
        step()
    captured = [t.grad for t in leaves]  # (the tensors the captured backward writes)
    gen = torch.Generator().manual_seed(77)
    for round_ in range(2):
        if round_ == 1:  # new values in the tensors the graphs read
            with torch.no_grad():
                for g in d["grid"]:
                    g.copy_(0.5 * torch.randn(g.shape, generator=gen))
        g_fwd.replay()
        g_bwd.replay()
        torch.cuda.synchronize()
        replayed = [g.clone() for g in captured]
        eager = forward()
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1]), f"round {round_}: replayed forward != eager"
        step()
        for i, (a, t) in enumerate(zip(replayed, leaves)):
            _worst(f"round {round_}: replayed gradient {i} vs eager", a, t.grad.cpu())
        assert torch.equal(replayed[-1], leaves[-1].grad)  # (the point gradient is stored, not accumulated: bit for bit)
    assert float((out[0].cpu().double() - c["op"]).abs().max()) > 1e-3  # (the second round really saw other grids)


def test_memory_is_the_two_results():
    """a no-grad eval_decoder_at_points over 262 144 points allocates its two results and (allocator rounding aside) nothing else: the
    bound of tests/test_gpu_scaffold.py::test_memory_is_the_result_plus_one_byte_per_point"""
    dev = _dev()
    mod, grids, _, _, _, _ = _module_inputs(dev)
    dg = [g.to(dev) for g in grids]
    R, N = 512, 512
    gen = torch.Generator().manual_seed(5)
    pts = (torch.rand(R, N, 3, generator=gen) * 2.4 - 1.2).to(dev)
    idx = torch.randint(0, 2, (R,), generator=gen).to(dev)
    enc = torch.randn(R, mod.rays_encoding_dim, generator=gen).to(dev)
    with torch.no_grad():
        mod.eval_decoder_at_points(pts[:1], idx[:1], enc[:1], dg)  # (library, kernels and the cached layer widths are loaded)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        op, col = mod.eval_decoder_at_points(pts, idx, enc, dg)
        torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated(dev) - before
    results = 4 * R * N * (1 + 3)
    print(f"peak extra memory {extra} bytes for results of {results}")
    assert op.shape == (R, N) and col.shape == (R, N, 3)
    assert extra <= 1.25 * results + 64 * 1024, f"{extra} bytes beyond the inputs for {results} bytes of results"

"""GPU tests of the module front-ends and of ABI 0.2's additions: module-level parity against fixtures made by the
REFERENCE's own modules, the fused ray-embedding kernels and bg / alpha epilogue (f3), zero-copy
grid-lists (f4), and the ray-sharded path driven through the real autograd functions by two ranks on one GPU."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib, grids as lp_grids
from lightplane_amd.modules import _RayEmbeddingFunction
from tests.synth import (MODULE_RENDERER_CASES, RENDERER_CASES, SPLATTER_CASES, grid_sizes_for, module_renderer_inputs,
                         random_rays)
from tests.test_gpu_parity import _assert_close, _dev, _rays_to, run_hip_mlp_splatter, run_hip_renderer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_module(spec, z, dev):
    mod = lp.LightplaneRenderer(**spec["ctor"]).to(dev)
    with torch.no_grad():
        mod.mlp_params.copy_(torch.from_numpy(z["state__mlp_params"]).to(dev))
        mod.harmonic_ray_embedding_linear.weight.copy_(torch.from_numpy(z["state__harmonic_ray_embedding_linear.weight"]).to(dev))
        mod.harmonic_ray_embedding_linear.bias.copy_(torch.from_numpy(z["state__harmonic_ray_embedding_linear.bias"]).to(dev))
    np.testing.assert_allclose(mod.bg_color.cpu().numpy(), z["state__bg_color"], rtol=0, atol=0)
    return mod


def _run_module(mod, spec, dev):
    sizes, grids, rays, up, _ = module_renderer_inputs(spec)
    gs = [g.to(dev).clone().requires_grad_(True) for g in grids]
    out = mod(_rays_to(rays, dev), gs)
    mod.zero_grad()
    sum((o * u.to(dev)).sum() for o, u in zip(out, up)).backward()
    return out, gs


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "torch_ops"])
@pytest.mark.parametrize("name", list(MODULE_RENDERER_CASES))
def test_module_renderer_matches_reference_module(name, fused, golden_dir):
    """LightplaneRenderer.forward (harmonic embedding -> Linear -> render -> background / alpha) against numbers the
    reference's LightplaneRenderer(use_naive_impl=True) produced (renderer_module.py:419-563): outputs and the gradients of
    mlp_params, the embedding's Linear layer and the grids.  Both the fused path (2 launches) and the PyTorch op chain."""
    dev = _dev()
    spec = MODULE_RENDERER_CASES[name]
    z = np.load(os.path.join(golden_dir, f"module_renderer__{name}.npz"))
    old = lp.config.fused_module_ops
    lp.config.fused_module_ops = fused
    try:
        mod = _build_module(spec, z, dev)
        out, gs = _run_module(mod, spec, dev)
    finally:
        lp.config.fused_module_ops = old
    for nm, o in zip(("ray_length", "alpha", "feature"), out):
        _assert_close(f"{name}: {nm}", o, z[nm])
    _assert_close(f"{name}: grad_mlp_params", mod.mlp_params.grad, z["grad_mlp_params"])
    _assert_close(f"{name}: grad_linear_weight", mod.harmonic_ray_embedding_linear.weight.grad, z["grad_linear_weight"])
    _assert_close(f"{name}: grad_linear_bias", mod.harmonic_ray_embedding_linear.bias.grad, z["grad_linear_bias"])
    for i, g in enumerate(gs):
        _assert_close(f"{name}: grad_grid{i}", g.grad, z[f"grad_grid{i}"])


def test_module_splatter_matches_reference_module(golden_dir):
    dev = _dev()
    z = np.load(os.path.join(golden_dir, "module_splatter.npz"))
    gen = torch.Generator().manual_seed(41)
    mod = lp.LightplaneSplatter(num_samples=9, grid_chn=16, mask_out_of_bounds_samples=True)
    rays = random_rays(gen, 40, 2, 16)
    rays.encoding = torch.rand(40, 16, generator=gen)
    out_sizes = grid_sizes_for((2, 6, 5, 7, 16), True)
    up = [torch.randn(*s, generator=gen) for s in out_sizes]
    r = _rays_to(rays, dev, True)
    out = mod(r, out_sizes)
    sum((o * u.to(dev)).sum() for o, u in zip(out, up)).backward()
    for i, o in enumerate(out):
        _assert_close(f"out{i}", o, z[f"out{i}"])
    _assert_close("grad_encoding", r.encoding.grad, z["grad_encoding"])


# (the last four: tests/ragged_cases.py EMBEDDING_CASES -- widths that are no multiple of 4, the narrowest one, the largest LDS tile)
@pytest.mark.parametrize("n_h,e,n", [(3, 32, 1000), (0, 16, 257), (10, 64, 33), (2, 20, 5), (3, 3, 257), (1, 1, 5), (0, 33, 64), (10, 85, 300)])
def test_ray_embedding_kernel_matches_torch_ops(n_h, e, n):
    """lp_ray_embedding_{forward,backward} == Linear(calc_harmonic_embedding(normalize(d))) and its autograd gradients."""
    dev = _dev()
    gen = torch.Generator().manual_seed(n_h * 100 + e)
    d = (torch.randn(n, 3, generator=gen) * torch.rand(n, 1, generator=gen) * 3).to(dev)
    lin = torch.nn.Linear(3 + 6 * n_h, e).to(dev)
    up = torch.randn(n, e, generator=gen).to(dev)
    ref = lin(lp.calc_harmonic_embedding(torch.nn.functional.normalize(d, dim=-1), n_h))
    (ref * up).sum().backward()
    gw, gb = lin.weight.grad.clone(), lin.bias.grad.clone()
    lin.zero_grad()
    out = _RayEmbeddingFunction.apply(d, lin.weight, lin.bias, n_h)
    (out * up).sum().backward()
    _assert_close("embedding", out, ref.detach().cpu().numpy(), 2e-5)  # sin(d 2^9): argument reduction differs
    _assert_close("grad weight", lin.weight.grad, gw.cpu().numpy(), 5e-5)
    _assert_close("grad bias", lin.bias.grad, gb.cpu().numpy(), 5e-5)


def test_grid_lists_are_zero_copy(monkeypatch):
    """A list of grids reaches the kernels through per-grid base pointers (LpGrid.data): nothing is concatenated
    (reference misc_utils.py:42-45 copies the list every call), the gradients are written into per-grid buffers, and the
    results equal the flat-tensor input."""
    dev = _dev()

    def boom(*a, **k):
        raise AssertionError("a grid-list was flattened (torch.cat) on the list path")

    for case_name in ("triplane_plus_voxel", "colorgrid_c32_mixed", "triplane_h64_c32"):
        d = next(c for c in RENDERER_CASES if c.name == case_name).build()
        for kernel in (_lib.LP_KERNEL_GENERIC, _lib.LP_KERNEL_AUTO):
            # flat input first (flatten_grid is the user's explicit call here)
            rays = _rays_to(d["rays"], dev, True)
            dec = d["decoder"]
            params = dec.mlp_params.to(dev).clone().requires_grad_(True)
            hdec = lp.DecoderParams(params, dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
            flat, sizes = lp.flatten_grid([g.to(dev) for g in d["grids"]])
            flat = flat.clone().requires_grad_(True)
            cflat, csizes = None, None
            if d["color_grids"] is not None:
                cflat, csizes = lp.flatten_grid([g.to(dev) for g in d["color_grids"]])
                cflat = cflat.clone().requires_grad_(True)
                csizes = csizes.tolist()
            scaffold = None if d["scaffold"] is None else d["scaffold"].to(dev)
            out_f = lp.lightplane_renderer(rays, flat, hdec, grid_sizes=sizes.tolist(), color_grid=cflat,
                                           color_grid_sizes=csizes, scaffold=scaffold, kernel=kernel, **d["cfg"])
            g_len, g_nlt, g_feat = (t.to(dev) for t in d["upstream"])
            ((out_f[0] * g_len).sum() + (out_f[1] * g_nlt).sum() + (out_f[2] * g_feat).sum()).backward()
            # list input with the flattening helpers booby-trapped
            with monkeypatch.context() as m:
                m.setattr(lp_grids, "_flatten_only", boom)
                m.setattr(lp_grids, "flatten_grid", boom)
                out_l, gp, ge, gg, gc = run_hip_renderer(d, dev, kernel)
            for a, b in zip(out_l, out_f):
                assert torch.equal(a, b), f"{case_name}: list and flat inputs give different outputs"
            want = torch.cat([g.reshape(-1, g.shape[-1]) for g in gg], dim=0)
            _assert_close(f"{case_name}: grid grads (list vs flat)", flat.grad, want.cpu().numpy(), 2e-5)
            if gc is not None:
                want = torch.cat([g.reshape(-1, g.shape[-1]) for g in gc], dim=0)
                _assert_close(f"{case_name}: colour grid grads (list vs flat)", cflat.grad, want.cpu().numpy(), 2e-5)
            _assert_close(f"{case_name}: params grads", params.grad, gp.cpu().numpy(), 2e-5)
    # MLP-Splatter input grid-list
    ds = next(c for c in SPLATTER_CASES if c.name == "mlp2_triplane_c16").build()
    with monkeypatch.context() as m:
        m.setattr(lp_grids, "_flatten_only", boom)
        out, ge, gp, gin = run_hip_mlp_splatter(ds, dev)
    rays = _rays_to(ds["rays"], dev, True)
    flat, sizes = lp.flatten_grid([g.to(dev) for g in ds["in_grids"]])
    flat = flat.clone().requires_grad_(True)
    mlp = lp.SplatterParams(ds["mlp"].mlp_params.to(dev).clone().requires_grad_(True), ds["mlp"].n_hidden)
    out_f = lp.lightplane_mlp_splatter(rays, ds["out_sizes"], mlp, flat, input_grid_sizes=sizes.tolist(), **ds["cfg"])
    sum((o * u.to(dev)).sum() for o, u in zip(out_f, ds["upstream"])).backward()
    for a, b in zip(out, out_f):
        _assert_close("mlp-splatter out (list vs flat)", a, b.detach().cpu().numpy(), 2e-6)
    want = torch.cat([g.reshape(-1, g.shape[-1]) for g in gin], dim=0)
    _assert_close("mlp-splatter input grid grads (list vs flat)", flat.grad, want.cpu().numpy(), 2e-5)


def test_fused_epilogue_matches_torch_ops_with_grads():
    """Background compositing + alpha inside the render kernel and its backward == the PyTorch op chain, all gradient
    families, for both alpha flavours and both kernel selections (cases of different kernel families)."""
    dev = _dev()
    from lightplane_amd.renderer import _render
    for case_name in ("triplane_basic", "voxel_deep", "triplane_h64_c32", "voxel_inf_contract"):
        d = next(c for c in RENDERER_CASES if c.name == case_name).build()
        n, cc = d["rays"].n_rays, d["decoder"].color_chn
        gen = torch.Generator().manual_seed(5)
        bg = torch.rand(cc, generator=gen).to(dev)
        g_alpha = torch.randn(n, generator=gen).to(dev)
        g_len, _, g_feat = (t.to(dev) for t in d["upstream"])
        for mode in (1, 2):
            res = []
            for fused in (True, False):
                rays = _rays_to(d["rays"], dev, True)
                dec = d["decoder"]
                params = dec.mlp_params.to(dev).clone().requires_grad_(True)
                hdec = lp.DecoderParams(params, dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, cc)
                gs = [g.to(dev).clone().requires_grad_(True) for g in d["grids"]]
                if fused:
                    ray_length, _, feature, alpha = _render(rays, gs, hdec, bg_color=bg, alpha_mode=mode, **d["cfg"])
                else:
                    ray_length, nlt, feature = lp.lightplane_renderer(rays, gs, hdec, **d["cfg"])
                    t = torch.exp(-nlt)
                    feature = feature + t[:, None] * bg
                    alpha = -nlt if mode == 2 else 1 - t
                ((ray_length * g_len).sum() + (alpha * g_alpha).sum() + (feature * g_feat).sum()).backward()
                res.append((ray_length, alpha, feature, params.grad, rays.encoding.grad, [g.grad for g in gs]))
            (l0, a0, f0, p0, e0, g0), (l1, a1, f1, p1, e1, g1) = res
            _assert_close(f"{case_name}/{mode}: alpha", a0, a1.detach().cpu().numpy(), 2e-6)
            _assert_close(f"{case_name}/{mode}: feature", f0, f1.detach().cpu().numpy(), 2e-6)
            _assert_close(f"{case_name}/{mode}: grad params", p0, p1.cpu().numpy(), 3e-5)
            _assert_close(f"{case_name}/{mode}: grad encoding", e0, e1.cpu().numpy(), 3e-5)
            for x, y in zip(g0, g1):
                _assert_close(f"{case_name}/{mode}: grad grid", x, y.cpu().numpy(), 3e-5)


def test_device_and_dtype_checks_raise_python_errors():
    """A CPU-resident mlp_params (LightplaneRenderer builds its parameters on the CPU: a forgotten .to(device)), rays on
    the CPU or float64 geometry raise AssertionError before any launch instead of faulting the GPU."""
    dev = _dev()
    d = RENDERER_CASES[0].build()
    dec = d["decoder"]
    rays = _rays_to(d["rays"], dev)
    grids = [g.to(dev) for g in d["grids"]]
    with pytest.raises(AssertionError, match="mlp_params"):
        lp.lightplane_renderer(rays, grids, dec, **d["cfg"])  # dec.mlp_params is on the CPU
    hdec = lp.DecoderParams(dec.mlp_params.to(dev), dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
    with pytest.raises(AssertionError, match="rays"):
        lp.lightplane_renderer(d["rays"], grids, hdec, **d["cfg"])  # rays on the CPU
    r64 = copy.copy(rays)
    r64.origins = rays.origins.double()
    with pytest.raises(AssertionError, match="float32"):
        lp.lightplane_renderer(r64, grids, hdec, **d["cfg"])
    ds = SPLATTER_CASES[0].build()
    rs = _rays_to(ds["rays"], dev)
    rs.near = ds["rays"].near  # CPU
    with pytest.raises(AssertionError, match="near"):
        lp.lightplane_splatter(rs, ds["out_sizes"], **ds["cfg"])


def test_rccl_collectives_on_a_one_rank_group():
    """RCCL (backend "nccl") executes the collectives of lightplane_amd/parallel.py on this GPU: the private coalescing
    context, reduce-scatter + all-gather on views of one buffer, the in-place all-reduce inside a Renderer backward
    (tests/nccl_worker.py; a one-rank group, because the build has no multi-GPU node)."""
    worker = os.path.join(ROOT, "tests", "nccl_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29900 + (os.getpid() % 90)), HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, worker], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0 and "RCCL_1RANK_OK" in out, out[-4000:]


def test_two_rank_ray_shards_equal_single_process():
    """The multi-GPU path end to end with the REAL autograd functions: two ranks (gloo, both on this GPU) each render /
    splat half of the rays; the all-reduced gradients / the all-reduced splat equal the single-process result."""
    worker = os.path.join(ROOT, "tests", "dist_worker.py")
    port = 29600 + (os.getpid() % 300)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), worker],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    out = r.stdout.decode()
    assert r.returncode == 0 and "DIST_OK" in out, out[-4000:]


def test_graphed_renderer_replays_the_module_step():
    """lightplane_amd.graphs.graphed_renderer: forward + backward of a LightplaneRenderer call captured into HIP graphs
    (torch.cuda.make_graphed_callables) and replayed on NEW ray / grid values: outputs and gradients of the grids and of
    the module's parameters equal the eager call's."""
    from lightplane_amd.graphs import graphed_renderer
    from tests.synth import grid_sizes_for, random_grids, random_rays
    dev = torch.device("cuda:0")
    old = lp.config.check_inputs
    lp.config.check_inputs = False
    try:
        torch.manual_seed(0)
        mod = lp.LightplaneRenderer(num_samples=24, color_chn=3, grid_chn=16, mlp_hidden_chn=32, gain=2.0, opacity_init_bias=-1.0,
                                    ray_embedding_num_harmonics=3, bg_color=0.2).to(dev)
        with torch.no_grad():
            mod.mlp_params.mul_(4.0)
        gen = torch.Generator().manual_seed(3)
        sizes = grid_sizes_for((2, 8, 9, 10, 16), True)

        def inputs(seed):
            g = torch.Generator().manual_seed(seed)
            grids = [x.to(dev).requires_grad_(True) for x in random_grids(g, sizes)]
            rays = random_rays(g, 300, 2, None).to(dev)
            up = [torch.randn(300, generator=g).to(dev), torch.randn(300, generator=g).to(dev), torch.randn(300, 3, generator=g).to(dev)]
            return rays, grids, up

        rays0, grids0, _ = inputs(1)
        fn = graphed_renderer(mod, rays0, grids0)
        for seed in (2, 3):
            rays, grids, up = inputs(seed)
            mod.zero_grad()
            out = fn(rays, grids)
            sum((o * u).sum() for o, u in zip(out, up)).backward()
            got = [o.detach().clone() for o in out] + [g.grad.clone() for g in grids] + [p.grad.clone() for p in mod.parameters()]
            grids_e = [g.detach().clone().requires_grad_(True) for g in grids]
            mod.zero_grad()
            out_e = mod(rays, grids_e)
            sum((o * u).sum() for o, u in zip(out_e, up)).backward()
            want = [o.detach() for o in out_e] + [g.grad for g in grids_e] + [p.grad for p in mod.parameters()]
            for i, (a, b) in enumerate(zip(got, want)):
                scale = float(b.abs().max()) + 1e-30
                assert float((a - b).abs().max()) / scale <= 2e-5, (seed, i)
    finally:
        lp.config.check_inputs = old


def test_bench_cfg5_two_ranks_on_one_gpu():
    """bench.py --workload cfg5 (splat shard -> sum over ranks -> normalise -> ray-sharded render -> gradient all-reduce ->
    splat backward) with two gloo ranks on this GPU, at toy sizes: the line the driver's 2 / 4 / 8-GPU runs would print."""
    import json
    port = 29900 + (os.getpid() % 90)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), CFG5_VIEWS="2", CFG5_IMG="48", CFG5_GRID="32",
               CFG5_ROWS="8", CFG5_S="32")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "cfg5", "--backend",
                        "gloo", "--steps", "2", "--warmup", "1", "--no-cpu-baseline"],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    out = r.stdout.decode()
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and lines, out[-4000:]
    res = json.loads(lines[-1])
    assert res["n_gpus"] == 2 and res["value"] > 0 and "cfg5" in res["config"]["workload"]
    assert res["config"]["rays_per_gpu"] == 2 * 48 * 48 + 8 * 1920


def test_bench_default_command_two_ranks_on_one_gpu():
    """The multi-GPU command with every leg -- `torch.distributed.run ... bench.py --gpus N --steps K --warmup W --full`, default
    workload -- with two gloo ranks on this GPU: the headline line with the sharded 1080p legs in `extras` (barrier + max over ranks),
    the roofline / binding blocks looked up by rank 0 without a collective (the other rank must not wait for it forever)."""
    import json
    port = 29800 + (os.getpid() % 90)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LP_BENCH_EXTRAS_TIMEOUT="400")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--steps", "5",
                        "--warmup", "2", "--full"],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    out = r.stdout.decode()
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and lines, out[-4000:]
    res = json.loads(lines[-1])
    assert res["n_gpus"] == 2 and res["value"] > 0 and res["scaling"] == "weak" and res["steps"] == 5
    assert res["roofline"]["dominant_kernel"].startswith("lp::renderer_bwd_bf3<16")
    assert "extras_error" not in res and set(res["extras"]) == {"renderer_1080p_s128", "renderer_cfg4_shard"}
    for leg in res["extras"].values():
        assert leg["n_gpus"] == 2 and leg["Mrays_per_s_fwd_bwd"] > 0, leg
    assert "cpu_baseline" not in res  # reported at N = 1 only


def test_bench_gpus_2_as_a_plain_process():
    """`python bench.py --gpus 2` WITHOUT a launcher (no WORLD_SIZE in the environment): bench.py re-launches itself as two ranks
    through torch.distributed.run (gloo here: two ranks share this GPU) and rank 0 prints the line (round-4 review, missing 5)."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--steps", "3", "--warmup", "1",
                        "--no-extras"], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    out = r.stdout.decode()
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, out[-4000:]
    res = json.loads(lines[-1])
    assert res["n_gpus"] == 2 and res["value"] > 0 and res["steps"] == 3 and "error" not in res
    assert res["config"]["rays_per_gpu"] == 65536 and "dp2" in res["config"]["parallelism"]


def test_bench_plain_run_dumps_the_last_timed_step(tmp_path):
    """`bench.py --steps K --warmup W --dump-outputs DIR`: the line is the headline alone (K timed steps, ms_per_step, no --full
    block), and DIR holds the outputs and input gradients of the cfg-2 step as float32 .npy files that equal one step of the same
    seeded workload rebuilt here."""
    import importlib.util
    import json
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(d)], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, out[-4000:]
    res = json.loads(lines[0])
    assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0 and res["unit"] == "Mrays/s" and res["dtype"] == "f32"
    assert abs(res["value"] - 65536 / res["ms_per_step"] / 1e3) <= 1e-3 * res["value"] + 1e-3
    assert not {"fwd_ms", "bwd_ms", "roofline", "peak_bwd_mem_mb", "extras", "cpu_baseline"} & set(res), sorted(res)

    spec = importlib.util.spec_from_file_location("lp_bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    old = lp.config.check_inputs
    lp.config.check_inputs = False
    try:
        wl = bench.RendererWorkload("cfg2", 0, torch.device("cuda:0"), None, _lib.LP_KERNEL_AUTO)
        want = {k: v.detach().cpu().numpy() for k, v in wl.results(wl.step()).items()}
    finally:
        lp.config.check_inputs = old
    assert sorted(p.name for p in d.iterdir()) == sorted(k + ".npy" for k in want)
    assert sum(p.stat().st_size for p in d.iterdir()) <= 64e6
    for k, w in want.items():
        got = np.load(d / (k + ".npy"))
        assert got.dtype == np.float32 and got.shape == w.shape, (k, got.dtype, got.shape)
        scale = float(np.abs(w).max()) + 1e-30
        assert float(np.abs(got - w).max()) <= 1e-5 * scale, k  # (grid-gradient atomics: summation order may differ per run)


def test_backward_with_offloaded_saved_tensors():
    """Saved-tensor hooks (CPU offloading, checkpointing) hand the backward NEW tensors: the argument block the backward
    re-uses from the forward must take its pointers from them, not from the forward's addresses."""
    from tests.synth import RENDERER_CASES
    from tests.test_gpu_parity import run_hip_renderer
    dev = torch.device("cuda:0")
    for name in ("triplane_plus_voxel", "voxel_c32_color1"):  # a grid-list of several tensors; S = 37: segment records saved too
        d = next(c for c in RENDERER_CASES if c.name == name).build()
        ref = run_hip_renderer(d, dev, _lib.LP_KERNEL_AUTO)
        with torch.autograd.graph.save_on_cpu():
            got = run_hip_renderer(d, dev, _lib.LP_KERNEL_AUTO)
        for a, b in zip([ref[1], ref[2]] + list(ref[3]), [got[1], got[2]] + list(got[3])):
            assert torch.allclose(a, b, rtol=1e-5, atol=1e-7 * float(a.abs().max()) + 1e-12), name

"""The FORWARD of deep hidden-64 decoders on the matrix cores (lp_renderer_forward_ws: family 3 with resident weight images, family 4
with streamed ones) against the reference's golden, the fp64 oracle and the shape-generic kernel it replaces; the mixed training
step (this forward, shape-generic backward) as the proof that the checkpoints it writes are the ones that backward reads.

Tolerance: the project's 1e-4 of the largest entry, no allowance."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib
from oracle import lightplane_oracle as O
from tests.synth import RENDERER_CASES, RendererCase, grid_sizes_for, pinhole_rays, random_decoder, random_grids
from tests.test_gpu_parity import _assert_close, _dev, forced_oracle_check

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _switch_on():
    old = lp.config.deep_forward_mfma
    lp.config.deep_forward_mfma = True
    yield
    lp.config.deep_forward_mfma = old


def _fwd(d, dev, kernel=_lib.LP_KERNEL_AUTO, **extra):
    rays = copy.copy(d["rays"])
    for f in ("directions", "origins", "grid_idx", "near", "far", "encoding"):
        setattr(rays, f, getattr(rays, f).to(dev))
    dec = copy.copy(d["decoder"])
    dec.mlp_params = dec.mlp_params.to(dev)
    grids = [g.to(dev) for g in d["grids"]]
    cg = None if d["color_grids"] is None else [g.to(dev) for g in d["color_grids"]]
    sc = None if d["scaffold"] is None else d["scaffold"].to(dev)
    with torch.no_grad():
        out = lp.lightplane_renderer(rays, grids, dec, scaffold=sc, color_grid=cg, kernel=kernel, **d["cfg"], **extra)
    torch.cuda.synchronize()
    return [o.cpu() for o in out[:3]]


def _oracle64(d, idx=None, chunk=1024):
    """fp64 oracle forward (chunked over rays, 16 threads)."""
    F = torch.float64
    rays = d["rays"] if idx is None else d["rays"][idx]
    dec = copy.copy(d["decoder"])
    dec.mlp_params = dec.mlp_params.to(F)
    grids = [g.to(F) for g in d["grids"]]
    cg = None if d["color_grids"] is None else [g.to(F) for g in d["color_grids"]]
    sc = None if d["scaffold"] is None else d["scaffold"].to(F)
    old = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    outs = [[], [], []]
    try:
        with torch.no_grad():
            for lo in range(0, rays.n_rays, chunk):
                r = rays[lo:lo + chunk]
                for f in ("directions", "origins", "near", "far", "encoding"):
                    setattr(r, f, getattr(r, f).to(F))
                o = O.lightplane_renderer_naive(r, grids, dec, scaffold=sc, color_grid=cg, **d["cfg"])
                for k in range(3):
                    outs[k].append(o[k])
    finally:
        torch.set_num_threads(old)
    return [torch.cat(o) for o in outs]


def _family(d):
    return lp.forward_kernel_family(d["rays"], d["grids"], d["decoder"], color_grid=d["color_grids"],
                                    num_samples_inf=d["cfg"]["num_samples_inf"])


NAMES = ("ray_length", "neg_log_t", "feature")


def _check_case(d, dev, want_family, what):
    assert _family(d) == want_family, what
    new = _fwd(d, dev)
    lp.config.deep_forward_mfma = False
    off = _fwd(d, dev)
    gen = _fwd(d, dev, kernel=_lib.LP_KERNEL_GENERIC)
    lp.config.deep_forward_mfma = True
    ora = _oracle64(d)
    for n, a, b, c, o in zip(NAMES, new, off, gen, ora):
        print(f"{what} {n}: vs oracle {float((a.double() - o).abs().max() / max(float(o.abs().max()), 1e-6)):.3e}, "
              f"vs switch off {float((a - b).abs().max() / max(float(b.abs().max()), 1e-6)):.3e}")
        assert torch.equal(b, c), f"{what} {n}: the switch off is not the generic kernel bit for bit"
        _assert_close(f"{what} {n}/oracle", a, o.numpy())
        _assert_close(f"{what} {n}/switch off", a, b.numpy())


def test_reference_golden(golden_dir):
    dev = _dev()
    case = next(c for c in RENDERER_CASES if c.name == "voxel_deep342_h64_c32")
    d = case.build()
    assert _family(d) == 4
    z = np.load(os.path.join(golden_dir, f"renderer__{case.name}.npz"))
    out = _fwd(d, dev)
    for n, a in zip(NAMES, out):
        _assert_close(n + "/golden", a, z[n])


SHAPES = [(layers, C, tri) for layers in ((3, 2, 2), (3, 3, 3), (4, 4, 4)) for C in (16, 32, 64) for tri in (False, True)]


@pytest.mark.parametrize("layers,C,tri", SHAPES, ids=[f"{''.join(map(str, l))}_c{C}_{'tri' if t else 'vox'}" for l, C, t in SHAPES])
def test_shapes_against_oracle(layers, C, tri):
    c = RendererCase("deep", seed=100 + C + sum(layers), n_rays=300, grid_base=(2, 6, 7, 5, C), is_triplane=tri, n_layers=layers,
                     hidden=64, num_samples=21)
    _check_case(c.build(), _dev(), 3 if layers == (3, 2, 2) else 4, f"{layers} x 64, C = {C}, {'triplane' if tri else 'voxel'}")


VARIANTS = {
    "colour_grid_044": (dict(n_layers=(0, 4, 4), separate_color_grid=True, grid_base=(2, 5, 6, 7, 32)), 4),
    "colour_grid_044_c16_tri": (dict(n_layers=(0, 4, 4), separate_color_grid=True, grid_base=(2, 8, 8, 8, 16), is_triplane=True), 4),
    "uneven_414": (dict(n_layers=(4, 1, 4)), 4),
    "uneven_141": (dict(n_layers=(1, 4, 1)), 3),
    "batch3_grid_idx": (dict(grid_base=(3, 5, 6, 7, 32)), 4),
    "scaffold": (dict(scaffold_size=(4, 5, 3)), 4),
    "noise": (dict(noise_sigma=0.3, noise_seed=7), 4),
    "contract_inf3": (dict(contract=True, num_samples_inf=3), 4),
    "contract_inf256": (dict(contract=True, num_samples_inf=256, n_rays=70), 4),
    "mask_oob": (dict(mask_oob=True), 4),
    "color1": (dict(color_chn=1), 4),
    "color4": (dict(color_chn=4), 4),
    "rays40": (dict(n_rays=40), 4),
    "rays1000": (dict(n_rays=1000), 4),
    "rays4099": (dict(n_rays=4099, num_samples=12), 4),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_variants_against_oracle(name):
    kw, fam = VARIANTS[name]
    base = dict(seed=200 + len(name), n_rays=300, grid_base=(2, 5, 6, 7, 32), n_layers=(4, 4, 4), hidden=64, num_samples=17)
    base.update(kw)
    d = RendererCase(name, **base).build()
    # (1/4/1: 2 + 12 block images fit the LDS: resident; everything else here streams)
    _check_case(d, _dev(), fam, name)


def test_module_epilogue_bg_colour_and_alpha():
    """The fused background / alpha epilogue of the module runs inside the render kernel: the module's outputs on the new forward
    against the fp64 oracle (the oracle's march on the module's own ray encoding and decoder, then the reference's epilogue --
    feature + T * bg, alpha = 1 - T -- in fp64) and against the generic forward."""
    dev = _dev()
    gen = torch.Generator().manual_seed(5)
    sizes = grid_sizes_for((1, 12, 12, 12, 32), True)
    grids = [g.to(dev) for g in random_grids(gen, sizes)]
    rays = pinhole_rays(20, 25, gen=gen)
    for f in ("directions", "origins", "grid_idx", "near", "far"):
        setattr(rays, f, getattr(rays, f).to(dev))
    rays.encoding = None
    torch.manual_seed(3)
    bg = (0.3, 0.6, 0.9)
    mod = lp.LightplaneRenderer(num_samples=24, color_chn=3, grid_chn=32, mlp_hidden_chn=64, mlp_n_layers_opacity=4, mlp_n_layers_trunk=4,
                                mlp_n_layers_color=4, bg_color=bg, opacity_init_bias=0.0).to(dev)
    F = torch.float64
    with torch.no_grad():
        dec = mod.get_decoder_params()
        assert lp.forward_kernel_family(rays, grids, dec) == 4
        new = [o.cpu() for o in mod(rays, grids)[:3]]
        lp.config.deep_forward_mfma = False
        old = [o.cpu() for o in mod(rays, grids)[:3]]
        lp.config.deep_forward_mfma = True
        r = copy.copy(rays)
        r.encoding = mod._get_ray_encoding(rays.encoding, rays.directions)
        for f in ("directions", "origins", "near", "far", "encoding"):
            setattr(r, f, getattr(r, f).cpu().to(F))
        r.grid_idx = r.grid_idx.cpu()
        odec = copy.copy(dec)
        odec.mlp_params = dec.mlp_params.cpu().to(F)
        o_len, o_nlt, o_feat = O.lightplane_renderer_naive(r, [g.cpu().to(F) for g in grids], odec, num_samples=24, gain=float(mod.gain))
        T = torch.exp(-o_nlt)
        ora = [o_len, 1 - T, o_feat + T[..., None] * torch.tensor(bg, dtype=F)]
    for n, x, y, o in zip(("module ray length", "module alpha", "module feature"), new, old, ora):
        print(f"{n}: vs oracle {float((x.double() - o).abs().max() / max(float(o.abs().max()), 1e-6)):.3e}")
        _assert_close(n + "/oracle", x, o.numpy())
        _assert_close(n + "/generic", x, y.numpy())


def test_whole_step_golden_shape():
    d = next(c for c in RENDERER_CASES if c.name == "voxel_deep342_h64_c32").build()
    assert _family(d) == 4
    forced_oracle_check("voxel_deep342_h64_c32 (streamed forward, generic backward)", d, _dev())


def test_whole_step_444():
    d = RendererCase("deep444_step", seed=31, n_rays=200, grid_base=(2, 6, 6, 6, 32), is_triplane=True, n_layers=(4, 4, 4), hidden=64,
                     num_samples=19).build()
    assert _family(d) == 4
    forced_oracle_check("4/4/4 x 64 (streamed forward, generic backward)", d, _dev())


def _full_chip_inputs(n_rays_hw=(384, 384), S=128):
    gen = torch.Generator().manual_seed(11)
    sizes = grid_sizes_for((1, 128, 128, 128, 32), True)
    grids = [0.5 * g for g in random_grids(gen, sizes)]
    dec = random_decoder(gen, 4, 4, 4, 32, 64, 3, std=0.15)
    rays = pinhole_rays(*n_rays_hw, enc_dim=64, gen=gen)
    cfg = dict(num_samples=S, gain=1.0, num_samples_inf=0, mask_out_of_bounds_samples=False, contract_coords=False,
               inject_noise_sigma=0.0, inject_noise_seed=0)
    return dict(rays=rays, grids=grids, color_grids=None, decoder=dec, scaffold=None, cfg=cfg, sizes=sizes)


def test_full_chip_launch():
    """147 456 rays x 128 samples, triplane 128^2 x 32, 4/4/4 x 64: every ray against the generic forward; eight rays (one of each
    of the eight waves) of every 64th workgroup and of the last one against the fp64 oracle."""
    dev = _dev()
    d = _full_chip_inputs()
    n = d["rays"].n_rays
    assert n == 147456 and _family(d) == 4
    new = _fwd(d, dev)
    gen = _fwd(d, dev, kernel=_lib.LP_KERNEL_GENERIC)
    for nm, a, b in zip(NAMES, new, gen):
        _assert_close("full chip / generic " + nm, a, b.numpy())
    n_wg = (n + 255) // 256
    wgs = sorted(set(list(range(0, n_wg, 64)) + [n_wg - 1]))
    idx = torch.tensor([w * 256 + k for w in wgs for k in (0, 37, 74, 111, 148, 185, 222, 255) if w * 256 + k < n])
    ora = _oracle64(d, idx, chunk=16)
    for nm, a, o in zip(NAMES, new, ora):
        _assert_close("full chip / oracle " + nm, a[idx], o.numpy())


STOP_WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "deep_forward_stop_worker.py")
# the worker's own work is seconds (three forwards of 8 000 / 64 000 / 556 rays x 40 samples, two backwards of 556 rays); the limit
# leaves room for the start of a fresh process on a loaded machine (interpreter, torch, HIP initialisation, loading the code objects)
STOP_TIMEOUT_S = 240


def _run_stop_worker(layers, seed, family):
    """The early-termination launches in a fresh child process under a time limit: a desynchronised barrier of the workgroup-synchronous
    kernel would hang, and a hang has to end as a failed test, not as a blocked suite."""
    root = os.path.dirname(os.path.dirname(STOP_WORKER))
    r = subprocess.run([sys.executable, STOP_WORKER, ",".join(map(str, layers)), str(seed), str(family)], cwd=root,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=STOP_TIMEOUT_S)
    out = r.stdout.decode()
    print(out[-3000:])
    assert r.returncode == 0 and "DEEP_STOP_OK" in out, out[-4000:]


def test_early_termination_on_a_dense_scene():
    """stop_transmittance on a dense scene, 4/4/4 x 64, in a child process that has to return within STOP_TIMEOUT_S
    (tests/deep_forward_stop_worker.py): outputs and -- through the shape-generic backward, which reads one last-marched sample per
    64 rays -- gradients meet the bar of tests/test_gpu_parity.py::test_renderer_early_termination; every 64-ray wavefront's last marched
    sample (the closing pair of neg_log_t_ckpt) is the shape-generic forward's; one workgroup holds wavefronts that stop at different
    samples next to one that never stops, one workgroup stops as a whole, the last one is part-filled (556 rays)."""
    _run_stop_worker((4, 4, 4), 77, 4)


def test_resident_deep_decoder_with_early_termination():
    """3/2/2 x 64 (resident images) with early termination takes the workgroup-synchronous kernel too, without a ring."""
    _run_stop_worker((3, 2, 2), 78, 3)


def test_graph_capture():
    """The forward under no_grad, captured and replayed twice, gives the eager outputs bit for bit (the workspace is a torch allocation:
    no host sync, one stream, no parallel branches)."""
    dev = _dev()
    d = RendererCase("deep444_graph", seed=41, n_rays=2000, grid_base=(1, 8, 8, 8, 32), is_triplane=True, n_layers=(4, 4, 4), hidden=64,
                     num_samples=16).build()
    assert _family(d) == 4
    rays = copy.copy(d["rays"])
    for f in ("directions", "origins", "grid_idx", "near", "far", "encoding"):
        setattr(rays, f, getattr(rays, f).to(dev))
    dec = copy.copy(d["decoder"])
    dec.mlp_params = dec.mlp_params.to(dev)
    grids = [g.to(dev) for g in d["grids"]]
    old = lp.config.check_inputs
    lp.config.check_inputs = False  # (its device sync cannot be captured)
    try:
        with torch.no_grad():
            eager = [o.clone() for o in lp.lightplane_renderer(rays, grids, dec, **d["cfg"])[:3]]
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                lp.lightplane_renderer(rays, grids, dec, **d["cfg"])  # warm-up on the side stream
            torch.cuda.current_stream().wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = lp.lightplane_renderer(rays, grids, dec, **d["cfg"])[:3]
            for _ in range(2):
                for o in out:
                    o.zero_()
                g.replay()
                torch.cuda.synchronize()
                for n, a, b in zip(NAMES, out, eager):
                    assert torch.equal(a, b), f"replay differs from eager: {n}"
    finally:
        lp.config.check_inputs = old

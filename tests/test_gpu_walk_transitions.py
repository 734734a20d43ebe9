"""Every user of the run-merged scatter walks on the scripted batches of tests/walk_cases.py, against the fp64 oracle.

tests/test_walk_transitions_host.py proves without a GPU which transitions every launch below takes (run heads, carried columns, axis
election, batch entries, row aliases, the weight window and its base rule, axes the cell code cannot hold), that no single contribution
is smaller than four bars and that the fp32 oracle meets the fp64 oracle at 2e-5 there.

* plain Splatter forward, ``march_order="rays"`` and ``"samples"``: the UN-NORMALISED feature sums and the weight sums separately
  (``lp_splatter_forward`` on zero-filled buffers of the test's own, argument block filled by the front-end's own ``_fill_args``) against
  ``oracle.splatter_sums`` -- the feature walk and the weight walk are separate code, after ``features / clamp(weights)`` an error of one is
  diluted by the other and a common one cancels --; the sets of non-zero cells exactly; the normalised output; two runs within 2e-5;
* plain Splatter backward: one and several segments, the row-length hint with an image height that is a multiple of four and one that is not;
* MLP-Splatter (layer-looped family, ``SplatSrcLds``): outputs and all gradients through ``check_mlp_splatter``, with a voxel output
  (``splat_walk_vox``) and with [voxel, xy plane] (``splat_walk``, the Splatter's per-slot walk, from the LDS tile; the backward's
  ``scatter_grid<E, GM_GENERIC, false>`` runs the Renderer's written-out per-slot loop in two passes on the voxel input grid);
* tuned Renderer, both march orders, through ``forced_oracle_check``: on a voxel grid (``splat_walk_vox<.., SPLAT = false>`` of its gradient
  scatter), on a canonical triplane (``scatter_triplane``: sentinel rows) and on [voxel, xy plane] (the tail of ``scatter_grid``: rows and
  validity bits).

Bars, the project's own: 1e-4 of the tensor's largest entry against the fp64 oracle, 2e-5 between two runs / two launch orders."""
import copy
import ctypes

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib
from oracle import lightplane_oracle as O
from tests import walk_cases as WC
from tests.test_gpu_parity import REL_TOL, _assert_close, _dev, _rel_err, forced_oracle_check, rel_l2

pytestmark = pytest.mark.gpu

F64 = torch.float64
RUN_TO_RUN = 2e-5     # the order of fp32 atomics (tests/test_gpu_layouts.py)
_ORACLE = {}


def _oracle(name, C, form):
    """fp64 sums and normalised outputs of a launch; computed once, shared, never modified"""
    key = (name, C, form)
    if key not in _ORACLE:
        case = WC.CASES[name]
        r64 = WC.rays_as(WC.build_rays(case, C), F64)
        sizes, cfg = WC.grid_sizes(case, C, form), WC.splat_cfg(case)
        _ORACLE[key] = (O.splatter_sums(r64, sizes, **cfg), O.lightplane_splatter_naive(r64, sizes, **cfg))
    return _ORACLE[key]


def raw_sums(rays, sizes, cfg, order, dev):
    """(feature sums [rows, C], weight sums [rows], march order handed to the library) of one ``lp_splatter_forward`` launch"""
    from lightplane_amd.grids import make_grid_descs, sizes_to_list
    from lightplane_amd.splatter import _SplatterCfg, _fill_args, _prep_rays
    descs, channels, n_rows = make_grid_descs(sizes_to_list(sizes))
    c = _SplatterCfg(descs, channels, n_rows, int(cfg["num_samples"]), 0, bool(cfg["mask_out_of_bounds_samples"]), False, 1e-5, None)
    r = rays.to(dev)
    (c.march_order, c.row_length), ray_tensors = _prep_rays(r, descs[0].B, order, 0)
    enc = _lib.aligned(r.encoding.contiguous())
    feat = torch.zeros(n_rows, channels, device=dev, dtype=torch.float32)
    wgt = torch.zeros(n_rows, device=dev, dtype=torch.float32)
    a = _fill_args(c, *ray_tensors, enc)
    a.out.data = _lib.ptr(feat)
    a.out_feature, a.out_weight = _lib.ptr(feat), _lib.ptr(wgt)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().lp_splatter_forward(ctypes.byref(a), _lib.current_stream(dev)), "lp_splatter_forward")
    torch.cuda.synchronize(dev)
    return feat, wgt, int(a.march_order)


def _forward(name, C, form, order):
    dev, case = _dev(), WC.CASES[name]
    rays, sizes, cfg = WC.build_rays(case, C), WC.grid_sizes(case, C, form), WC.splat_cfg(case)
    tag = f"walk-transitions {name} C={C} {form} [{order}]"
    sums64, norm64 = _oracle(name, C, form)
    feat, wgt, march = raw_sums(rays, sizes, cfg, order, dev)
    # never a silent fall-back: the argument block says which forward walk the launcher takes (it has no other for these channel counts)
    assert march == (_lib.LP_MARCH_SAMPLES_PER_WAVE if order == "samples" else _lib.LP_MARCH_RAYS_PER_WAVE), tag
    feat2, wgt2, _ = raw_sums(rays, sizes, cfg, order, dev)
    row = 0
    for g, (gs, (f64, w64)) in enumerate(zip(sizes, sums64)):
        n = gs[0] * gs[1] * gs[2] * gs[3]
        f, w, f2, w2 = feat[row:row + n], wgt[row:row + n], feat2[row:row + n], wgt2[row:row + n]
        row += n
        ef, ew = _rel_err(f, f64.numpy()), _rel_err(w, w64.numpy())
        print(f"{tag} grid {g}: feature sums {ef / REL_TOL:.3f} bars, weight sums {ew / REL_TOL:.3f} bars; run to run "
              f"{_rel_err(f2, f.cpu().numpy()):.2e} / {_rel_err(w2, w.cpu().numpy()):.2e}")
        _assert_close(f"{tag} grid {g}: feature sums", f, f64.numpy())
        _assert_close(f"{tag} grid {g}: weight sums", w, w64.numpy())
        got_f, want_f = (f != 0).any(dim=1).cpu(), (f64 != 0).any(dim=1)
        assert torch.equal(got_f, want_f), f"{tag} grid {g}: {int((got_f != want_f).sum())} rows differ in being touched (features)"
        got_w, want_w = (w != 0).cpu(), w64 != 0
        assert torch.equal(got_w, want_w), f"{tag} grid {g}: {int((got_w != want_w).sum())} cells differ in being touched (weights)"
        _assert_close(f"{tag} grid {g}: feature sums, second run", f2, f.cpu().numpy(), tol=RUN_TO_RUN)
        _assert_close(f"{tag} grid {g}: weight sums, second run", w2, w.cpu().numpy(), tol=RUN_TO_RUN)
    out = lp.lightplane_splatter(rays.to(dev), sizes, march_order=order, rays_per_row=0, **cfg)
    for g, (o, o64) in enumerate(zip(out, norm64)):
        print(f"{tag} grid {g}: normalised output {_rel_err(o, o64.numpy()) / REL_TOL:.3f} bars")
        _assert_close(f"{tag} grid {g}: normalised output", o, o64.numpy())


@pytest.mark.parametrize("name,C,form", WC.FORWARD_RAYS, ids=[f"{n}-c{C}-{f}" for n, C, f in WC.FORWARD_RAYS])
def test_splatter_forward_rays_per_wave(name, C, form):
    """C = 16: the one-axis walk and the weight windows; C = 32 / 64 on a voxel grid: the two-axis walk at 32 / 16 rays per wave; on a list
    [voxel, xy plane]: ``splat_walk_vox`` at two / four channels per lane and ``splat_walk``; C = 16 on a triplane"""
    _forward(name, C, form, "rays")


@pytest.mark.parametrize("name,C,form", WC.FORWARD_SAMPLES, ids=[f"{n}-c{C}-{f}" for n, C, f in WC.FORWARD_SAMPLES])
def test_splatter_forward_samples_per_wave(name, C, form):
    """the transposed march: the scripts are the rays -- dwelling, unit steps, every diagonal (taken as two unit steps), jumps, a ray
    that enters and leaves the grid inside one block of 32 samples, 33 / 40 samples (dead lanes in the last block)"""
    _forward(name, C, form, "samples")


def _backward(case, C, row, dev, upstream):
    rays = WC.build_rays(case, C).to(dev)
    rays = copy.copy(rays)
    rays.encoding = rays.encoding.clone().requires_grad_(True)
    sizes = WC.grid_sizes(case, C)
    (out,) = lp.lightplane_splatter(rays, sizes, march_order="rays", rays_per_row=row, **WC.splat_cfg(case))
    (out * upstream.to(dev)).sum().backward()
    return rays.encoding.grad


@pytest.mark.parametrize("name,C,row", WC.BACKWARD, ids=[f"{n}-c{C}-row{r}" for n, C, r in WC.BACKWARD])
def test_splatter_backward(name, C, row):
    """``splat_bwd_walk_kernel`` (8 rays per wave x blocks of 8 samples): ``grad_encoding`` against the fp64 oracle at 1e-4 of the largest
    entry and by relative L2; one segment (8 samples), several (33 / 40 samples), 2 x 4 pixel patches of an 8 x 8 and a 6 x 8 image --
    those also within 2e-5 of the run without the hint"""
    dev, case = _dev(), WC.CASES[name]
    sizes, cfg = WC.grid_sizes(case, C), WC.splat_cfg(case)
    gen = torch.Generator().manual_seed(77)
    up = torch.randn(*sizes[0], generator=gen)
    r64 = WC.rays_as(WC.build_rays(case, C), F64)
    r64.encoding = r64.encoding.clone().requires_grad_(True)
    (o64,) = O.lightplane_splatter_naive(r64, sizes, **cfg)
    (o64 * up.double()).sum().backward()
    want = r64.encoding.grad
    got = _backward(case, C, row, dev, up)
    tag = f"walk-transitions backward {name} C={C} row length {row}"
    print(f"{tag}: grad_encoding {_rel_err(got, want.numpy()) / REL_TOL:.3f} bars, relative L2 {rel_l2(got, want.numpy()):.2e}")
    _assert_close(f"{tag}: grad_encoding", got, want.numpy())
    assert rel_l2(got, want.numpy()) <= 1e-4, f"{tag}: grad_encoding relative L2 {rel_l2(got, want.numpy()):.3e}"
    if row:
        plain = _backward(case, C, 0, dev, up)
        _assert_close(f"{tag}: with against without the row-length hint", got, plain.cpu().numpy(), tol=RUN_TO_RUN)


MLP_IN_BASE = (5, 6, 7)     # (D, H, W) of the MLP-Splatter's voxel input grid


def _mlp_splatter(name, form):
    from tests.synth import random_grids, random_splatter_mlp
    from tests.test_gpu_coherent import check_mlp_splatter
    case = WC.CASES[name]
    gen = torch.Generator().manual_seed(5)
    in_sizes = [[case.base[0], *MLP_IN_BASE, 32]]
    out_sizes = WC.grid_sizes(case, 32, form)
    mlp = random_splatter_mlp(gen, 2, 32, 32, 32, std=0.2)
    d = dict(rays=WC.build_rays(case, 32), out_sizes=out_sizes, mlp=mlp, in_grids=random_grids(gen, in_sizes), in_sizes=in_sizes,
             cfg=WC.splat_cfg(case), upstream=[torch.randn(*s, generator=gen) for s in out_sizes])
    assert lp.mlp_splatter_kernel_family(out_sizes, mlp, in_sizes) == 3
    check_mlp_splatter(d, _dev(), _lib.LP_KERNEL_AUTO, f"walk-transitions MLP-Splatter {name} {form}")


@pytest.mark.parametrize("name", ["main", "main_mask"])
def test_mlp_splatter_on_the_scripted_batch(name):
    """The MLP-Splatter's walk (``splat_walk_vox`` reading its LDS tile, lp_splatter_mlp_loop.h) on the main scripted batch, without and
    with the out-of-bounds mask (dead lanes: a carry refused by validity): a two-layer hidden-32 MLP, 32 -> 32 channels, voxel output,
    layer-looped family; outputs and every gradient as ``check_mlp_splatter`` compares them"""
    _mlp_splatter(name, "voxel")


@pytest.mark.parametrize("name", ["main", "main_mask"])
def test_mlp_splatter_with_a_plane_among_its_outputs(name):
    """The same launch with [voxel, xy plane] outputs: the plane goes through the Splatter's per-slot walk (``splat_walk``: ``splat_walk_slots`` from the LDS
    tile and ``splat_walk_unit_weights``), and the backward scatters the gradient of the voxel input grid with the two-pass
    form of ``scatter_grid<E, GM_GENERIC, false>`` (tests/test_walk_transitions_host.py: which branches both take)"""
    _mlp_splatter(name, "voxel+xy")


RENDERER = [("main", 16, "rays"), ("main_mask", 32, "rays"), ("transposed_s40_mask", 16, "samples"), ("transposed_s33", 32, "samples"),
            ("long_z1500", 16, "rays")]
RENDERER_PLANES = [(n, C, o, form) for n, C, o in (("main", 16, "rays"), ("main_mask", 32, "rays"), ("transposed_s33", 32, "samples"))
                   for form in ("triplane", "voxel+xy")]


def renderer_inputs(name, C, form="voxel"):
    """A tuned-family Renderer launch on the scripted batch: the case's grid-list in ``form`` (one voxel grid of the case's size; a canonical
    triplane; the voxel grid and an xy plane), a 2/2/2 x 32 decoder"""
    from tests.synth import random_decoder, random_grids
    case = WC.CASES[name]
    gen = torch.Generator().manual_seed(9 + C)
    sizes = WC.grid_sizes(case, C, form)
    dec = random_decoder(gen, 2, 2, 2, C, 32, 3, std=0.2)
    rays = WC.build_rays(case, int(dec.n_hidden_color[0]))
    n = rays.n_rays
    cfg = dict(num_samples=case.num_samples, gain=2.0, num_samples_inf=0, mask_out_of_bounds_samples=case.mask, contract_coords=False,
               inject_noise_sigma=0.0, inject_noise_seed=0)
    up = (torch.randn(n, generator=gen), torch.randn(n, generator=gen), torch.randn(n, 3, generator=gen))
    return dict(rays=rays, grids=random_grids(gen, sizes), color_grids=None, decoder=dec, scaffold=None, cfg=cfg, sizes=sizes, upstream=up)


@pytest.mark.parametrize("name,C,order", RENDERER, ids=[f"{n}-c{C}-{o}" for n, C, o in RENDERER])
def test_tuned_renderer_gradient_scatter(name, C, order):
    """The tuned Renderer's gradient scatter is the same one-axis walk in the Renderer's convention: every entry of ``grad_grid`` (and every
    other tensor) at 1e-4 with the backward's own ReLU decisions forced onto the fp64 oracle; both march orders; one carrier on the
    1 500-cell axis"""
    _tuned_renderer(name, C, order, "voxel")


def _tuned_renderer(name, C, order, form):
    d = renderer_inputs(name, C, form)
    assert lp.kernel_family(d["rays"], d["grids"], d["decoder"]) == 1
    forced_oracle_check(f"walk-transitions Renderer {name} C={C} [{order}] {form}", d, _dev(), chunk=d["rays"].n_rays, march_order=order)
    last = _lib.lib().lp_debug_last_renderer_backward
    last.restype = ctypes.c_char_p
    assert (b"transposed march" in last()) == (order == "samples"), f"march_order={order!r} launched {last()}"  # never a silent fall-back


@pytest.mark.parametrize("name,C,order,form", RENDERER_PLANES, ids=[f"{n}-c{C}-{o}-{f}" for n, C, o, f in RENDERER_PLANES])
def test_tuned_renderer_gradient_scatter_on_planes(name, C, order, form):
    """The tuned Renderer's gradient scatter on plane grids, both march orders: a canonical triplane goes through ``scatter_triplane`` (the
    per-slot run loop with sentinel rows and the single-run fast path, one plane after the other); the list [voxel, xy plane] is
    ``GM_GENERIC`` -- the voxel grid takes the column walk, the plane the tail of ``scatter_grid`` (the same loop written out with rows and validity
    bits).  tests/test_walk_transitions_host.py: every launch has single-run wave-samples, several-run ones and, masked, dead runs between
    live ones"""
    _tuned_renderer(name, C, order, form)

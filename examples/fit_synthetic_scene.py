#!/usr/bin/env python
"""End-to-end check of the MI355X Renderer: fit a triplane + decoder to an analytic scene.

The target is a soft coloured ball rendered with a plain PyTorch emission-absorption march; the student is a
``LightplaneRenderer`` module (direction-dependent colours through the harmonic ray embedding) with three
plane grids as parameters, optimised with Adam on random rays.  The role of the reference's
examples/fit_single_scene.py training loop (:282-334) as a convergence check, on synthetic data because the
GPU boxes have no datasets.

    python examples/fit_synthetic_scene.py [--steps 300] [--rays 8192] [--stop-transmittance 0] [--tv-weight 0] [--upsample-steps 100,200]
                                            [--scaffold-steps 150,250] [--scaffold-size 64] [--export-pointcloud FILE.npy] [--clip-rays]
                                            [--export-mesh FILE.ply] [--mesh-size 64] [--mesh-level 1.0] [--modular]
                                            [--importance N] [--distortion-weight W] [--render-samples]

``--tv-weight w`` (> 0) adds ``w`` times the total variation of the three planes to the objective: its gradient is added to the
planes' ``.grad`` by one fused sweep after ``loss.backward()`` (``lp.add_grid_tv_grad_``); 0 leaves the run as it is without it.

``--upsample-steps 100,200`` fits coarse to fine (the reference example's schedule, examples/fit_single_scene.py): the planes start at
``res / 2^k`` for ``k`` listed steps, and before each of those steps ``lp.grid_up_sample`` doubles them -- one HIP sweep per plane on
the planes' own layout -- and the optimiser is rebuilt for the new tensors.  Without it the run is as it always was.

``--scaffold-steps 150,250`` rebuilds the occupancy scaffold before each of those steps, as the reference's training recipe does
periodically (examples/fit_single_scene.py ``update_scaffold_step``): ``renderer.calculate_scaffold`` on a ``--scaffold-size``^3 lattice
-- one fused lattice kernel plus a byte dilation -- and every render from then on, held-out evaluation included, skips the samples
the scaffold marks empty.  ``--scaffold-threshold`` is the opacity above which a lattice point counts as occupied (the module's default
1e-7 keeps nearly everything).  Without ``--scaffold-steps`` no scaffold is built or passed.

``--clip-rays`` clips every ray batch -- training and held-out -- to the span it can contribute on before the target and the student
are rendered: ``renderer.clip_rays`` walks the rays through the scaffold's cells (one fused kernel, ``lp.clip_rays_to_scaffold``) and
shrinks ``near`` / ``far`` to the occupied span, half a cell wider; before a scaffold exists the rays are clipped to the scene box.  Rays
that cross no occupied cell stay in the batch and render background in both.  The sample count stays, so the sample density rises by
``1 / mean_span_ratio``; the JSON line gains ``mean_span_ratio`` (mean of ``(far' - near') / (far - near)`` over the last training
batch) and ``hit_fraction``.  Without the flag the run is bit for bit what it is without this option.

``--export-pointcloud FILE.npy`` writes the fitted scene as a point cloud after the fit: the occupancy scaffold of a
``--scaffold-size``^3 lattice at ``--scaffold-threshold`` (no dilation) picks the occupied lattice points, ``renderer.eval_decoder_at_points``
-- one fused kernel, ``lp.lightplane_eval_mlp`` -- gives their opacity and their colour seen along ``-z``, and the file holds one
float32 row ``x y z | r g b | opacity`` per point.

``--export-mesh FILE.ply`` writes the fitted scene as a triangle mesh after the fit: ``renderer.extract_mesh`` -- the fused opacity
lattice of ``--mesh-size``^3 points, marching cubes on the GPU at the opacity ``--mesh-level`` (``lp.marching_cubes``) and the fused
point decoder for the vertex colours seen along ``-z`` -- and the file is an ASCII PLY with positions, normals and 8-bit colours.

``--modular`` renders the training batches through the modular march instead of the fused Renderer: ``renderer.ray_samples`` places
the samples, ``renderer.eval_decoder_at_points`` (``lp.lightplane_eval_mlp``) decodes them and ``lp.composite_samples`` integrates
them -- the same fit, with the per-sample tensors in the caller's hands (the JSON line gains ``modular``).  The held-out evaluation
stays on the fused Renderer, so the PSNR also says that the two paths agree.  Without the flag the run is untouched.

``--importance N`` (with ``--modular``) makes that march NeRF's coarse -> fine pass: the march above runs under ``no_grad`` and only for
its compositing weights (``composite_samples(..., return_weights=True)``), ``renderer.importance_samples`` draws ``N`` more samples per
ray from them (stratified, jittered with ``torch.rand``) and merges them into the coarse ones, and the fine pass over the
``num_samples + N`` samples is the one that is fitted (the JSON line gains ``importance``).  0 leaves the run as it is without it.

``--distortion-weight W`` (> 0, with ``--modular``) adds ``W`` times mip-NeRF 360's distortion loss of the fitted march to the objective:
``W * mean(lp.distortion_loss(weights, depths, deltas) / (far - near))`` on the weights ``composite_samples(..., return_weights=True)``
hands back -- one fused kernel, with gradients through the weights into the decoder and the planes (the JSON line gains
``distortion_weight`` and the first / last value of the term).  0 leaves the run as it is without it.

``--render-samples`` (with ``--modular``) runs the fitted march -- the fine pass with ``--importance`` -- through
``renderer.render_samples`` (``lp.render_samples``): the decoder and the compositing in one launch at the samples' depths, with no
points, opacity or colour tensor in between; the distortion loss then reads the weights that op hands back (the JSON line gains
``render_samples``).  The coarse pass of ``--importance`` stays on the chain.

Prints one JSON line with the first / last losses and the PSNR of a held-out ray batch.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lightplane_amd as lp  # noqa: E402


def scene(p):
    """density and colour of the analytic scene at points p [..., 3]"""
    r = p.norm(dim=-1)
    sigma = 25.0 * torch.sigmoid((0.55 - r) * 25.0)
    rgb = 0.5 + 0.5 * torch.sin(5.0 * p + torch.tensor([0.0, 2.0, 4.0], device=p.device))
    return sigma, rgb


def render_target(origins, directions, near, far, num_samples):
    t = torch.linspace(0.0, 1.0, num_samples, device=origins.device)
    depth = near[:, None] + (far - near)[:, None] * t[None]
    p = origins[:, None] + depth[..., None] * directions[:, None]
    sigma, rgb = scene(p)
    delta = torch.cat([(far - near)[:, None] / (num_samples - 1), depth[:, 1:] - depth[:, :-1]], dim=1)
    nlt = torch.cumsum(sigma * delta, dim=1)
    trans = torch.exp(-torch.cat([torch.zeros_like(nlt[:, :1]), nlt], dim=1))
    w = trans[:, :-1] - trans[:, 1:]
    return (w[..., None] * rgb).sum(1), 1.0 - trans[:, -1]


def random_rays(n, gen, dev):
    o = torch.randn(n, 3, generator=gen)
    o = 2.5 * o / o.norm(dim=-1, keepdim=True)
    tgt = torch.randn(n, 3, generator=gen)
    tgt = 0.8 * tgt / tgt.norm(dim=-1, keepdim=True) * torch.rand(n, 1, generator=gen) ** (1 / 3)
    d = tgt - o
    d = d / d.norm(dim=-1, keepdim=True)
    near, far = torch.full((n,), 1.2), torch.full((n,), 3.8)
    return lp.Rays(directions=d.to(dev), origins=o.to(dev), grid_idx=torch.zeros(n, dtype=torch.int32, device=dev),
                   near=near.to(dev), far=far.to(dev), encoding=None)


def heldout_psnr(renderer, grids, n_rays, num_samples, seed, dev, scaffold=None, clip_rays=False):
    rays = random_rays(n_rays, torch.Generator().manual_seed(seed + 1), dev)
    if clip_rays:
        rays, _ = renderer.clip_rays(rays, scaffold)
    with torch.no_grad():
        tgt_rgb, _ = render_target(rays.origins, rays.directions, rays.near, rays.far, num_samples)
        _, _, rgb = renderer(rays, list(grids), scaffold=scaffold)
        mse = float(((rgb - tgt_rgb) ** 2).mean())
    return -10.0 * math.log10(mse)


def render_modular(renderer, rays, grids, scaffold=None, importance=0, distortion=False, fused_fine=False):
    """``(alpha, rgb, distortion)`` of ``renderer(rays, grids)`` through ray_samples -> the decoder at points -> composite_samples
    (background 0); ``importance`` > 0: that march only for its weights, and the result from the samples ``importance_samples`` makes
    of them; ``distortion``: the mean distortion loss of the fitted march on distances normalised by ``far - near`` (else ``None``);
    ``fused_fine``: the fitted march runs through ``renderer.render_samples`` -- decoder and compositing in one launch at the samples'
    depths, without the per-sample tensors"""
    samples = renderer.ray_samples(rays)
    if importance > 0:
        with torch.no_grad():
            opacity, _ = renderer.eval_decoder_at_points(samples.points, rays.grid_idx, None, grids, scaffold=scaffold,
                                                         directions=rays.directions)
            weights = lp.composite_samples(opacity, None, samples.depths, samples.deltas, return_weights=True)[3]
            jitter = torch.rand(weights.shape[0], importance, device=weights.device)
        samples = renderer.importance_samples(rays, samples, weights, importance, jitter=jitter)
    if fused_fine:
        out = renderer.render_samples(rays, grids, samples, scaffold=scaffold, return_weights=distortion)
        dist = (lp.distortion_loss(out[3], samples.depths, samples.deltas) / (rays.far - rays.near)).mean() if distortion else None
        return out[1], out[2], dist
    opacity, color = renderer.eval_decoder_at_points(samples.points, rays.grid_idx, None, grids, scaffold=scaffold,
                                                     directions=rays.directions)
    if not distortion:
        _, nlt, rgb = lp.composite_samples(opacity, color, samples.depths, samples.deltas)
        return 1.0 - torch.exp(-nlt), rgb, None
    _, nlt, rgb, weights = lp.composite_samples(opacity, color, samples.depths, samples.deltas, return_weights=True)
    dist = (lp.distortion_loss(weights, samples.depths, samples.deltas) / (rays.far - rays.near)).mean()
    return 1.0 - torch.exp(-nlt), rgb, dist


def fit(steps=300, n_rays=8192, num_samples=96, res=64, chn=16, seed=0, stop_transmittance=0.0, verbose=False, tv_weight=0.0,
        upsample_steps=(), scaffold_steps=(), scaffold_size=64, scaffold_threshold=1e-7, export_pointcloud=None, clip_rays=False,
        export_mesh=None, mesh_size=64, mesh_level=1.0, on_fitted=None, modular=False, importance=0, distortion_weight=0.0,
        fused_fine=False):
    """``on_fitted(renderer, grids)``: called after the last step, before the exports, with the fitted module and its planes"""
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    lp.config.stop_transmittance = float(stop_transmittance)
    renderer = lp.LightplaneRenderer(num_samples=num_samples, color_chn=3, grid_chn=chn, mlp_hidden_chn=32,
                                     opacity_init_bias=-2.0, gain=1.0, bg_color=0.0).to(dev)
    upsample_steps = sorted(int(v) for v in upsample_steps)
    start_res = res >> len(upsample_steps)
    assert start_res >= 2 and start_res << len(upsample_steps) == res, f"res {res} cannot be halved {len(upsample_steps)} times"
    shapes = [(1, 1, start_res, start_res, chn), (1, start_res, 1, start_res, chn), (1, start_res, start_res, 1, chn)]
    grids = torch.nn.ParameterList([torch.nn.Parameter(0.1 * torch.randn(*s, generator=gen).to(dev)) for s in shapes])

    def make_opt():
        return torch.optim.Adam([{"params": grids.parameters(), "lr": 3e-2}, {"params": renderer.parameters(), "lr": 3e-3}])

    opt = make_opt()
    scaffold_steps = sorted(int(v) for v in scaffold_steps)
    scaffold, occupancy = None, []
    losses, tvs, dists, psnr_at_upsample = [], [], [], []
    for it in range(steps):
        if it in upsample_steps:
            psnr_at_upsample.append(heldout_psnr(renderer, grids, n_rays, num_samples, seed, dev, scaffold, clip_rays))
            new = lp.grid_up_sample([g.detach() for g in grids], upsample_factor=2.0)
            grids = torch.nn.ParameterList([torch.nn.Parameter(g) for g in new])
            opt = make_opt()  # new tensors: new optimiser state, as the reference example does
            if verbose:
                print(f"step {it:4d}  planes -> {tuple(grids[0].shape)}  held-out PSNR before {psnr_at_upsample[-1]:.2f} dB", flush=True)
        if it in scaffold_steps:
            scaffold = renderer.calculate_scaffold(list(grids), [1, scaffold_size, scaffold_size, scaffold_size], dev,
                                                   threshold=scaffold_threshold)
            occupancy.append(float(scaffold.mean()))
            if verbose:
                print(f"step {it:4d}  scaffold {tuple(scaffold.shape)}  occupied {occupancy[-1]:.3f}", flush=True)
        rays = random_rays(n_rays, gen, dev)
        if clip_rays:
            span = rays.far - rays.near
            rays, hit = renderer.clip_rays(rays, scaffold)
        with torch.no_grad():
            tgt_rgb, tgt_alpha = render_target(rays.origins, rays.directions, rays.near, rays.far, num_samples)
        if modular:
            alpha, rgb, dist = render_modular(renderer, rays, list(grids), scaffold, importance, distortion_weight > 0.0, fused_fine)
        else:
            _, alpha, rgb = renderer(rays, list(grids), scaffold=scaffold)
        loss = ((rgb - tgt_rgb) ** 2).mean() + 0.1 * ((alpha - tgt_alpha) ** 2).mean()
        if modular and distortion_weight > 0.0:
            loss = loss + distortion_weight * dist
            dists.append(float(dist.detach()))
        opt.zero_grad(set_to_none=True)
        loss.backward()
        if tv_weight > 0.0:
            tvs.append(lp.add_grid_tv_grad_(list(grids), [g.grad for g in grids], weight=tv_weight))
        opt.step()
        losses.append(float(loss.detach()))
        if verbose and (it % 50 == 0 or it == steps - 1):
            print(f"step {it:4d}  loss {losses[-1]:.5f}", flush=True)
    out = {"first_loss": sum(losses[:5]) / 5, "last_loss": sum(losses[-5:]) / 5,
           "heldout_psnr_db": heldout_psnr(renderer, grids, n_rays, num_samples, seed, dev, scaffold, clip_rays),
           "steps": steps, "rays_per_step": n_rays, "stop_transmittance": stop_transmittance}
    if modular:
        out.update(modular=True)
    if importance > 0:
        out.update(importance=importance)
    if fused_fine:
        out.update(render_samples=True)
    if distortion_weight > 0.0:
        out.update(distortion_weight=distortion_weight, first_distortion=dists[0], last_distortion=dists[-1])
    if upsample_steps:
        out.update(upsample_steps=upsample_steps, start_res=start_res, psnr_at_upsample_db=psnr_at_upsample,
                   grid_shapes=[list(g.shape) for g in grids])
    if scaffold_steps:
        out.update(scaffold_steps=scaffold_steps, scaffold_shape=list(scaffold.shape) if scaffold is not None else None,
                   scaffold_threshold=scaffold_threshold, scaffold_occupancy=occupancy)
    if clip_rays and steps > 0:
        out.update(mean_span_ratio=float(((rays.far - rays.near) / span).mean()), hit_fraction=float(hit.float().mean()))
    if tv_weight > 0.0:
        out.update(tv_weight=tv_weight, first_tv=float(tvs[0]), last_tv=float(tvs[-1]),
                   grads_finite=all(bool(torch.isfinite(g.grad).all()) for g in grids))
    if on_fitted is not None:
        on_fitted(renderer, list(grids))
    if export_pointcloud:
        cloud = pointcloud(renderer, list(grids), scaffold_size, scaffold_threshold, dev)
        np.save(export_pointcloud, cloud.cpu().numpy())
        out.update(pointcloud_file=export_pointcloud, pointcloud_points=int(cloud.shape[0]))
    if export_mesh:
        mesh = renderer.extract_mesh(list(grids), [1, mesh_size, mesh_size, mesh_size], level=mesh_level,
                                     view_directions=torch.tensor([[0.0, 0.0, -1.0]], device=dev))
        write_ply(export_mesh, mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy(), mesh.normals.cpu().numpy(),
                  mesh.colors.cpu().numpy())
        out.update(mesh_file=export_mesh, mesh_vertices=int(mesh.vertices.shape[0]), mesh_faces=int(mesh.faces.shape[0]),
                   mesh_level=mesh_level)
    return out


def write_ply(path, vertices, faces, normals, colors):
    """ASCII PLY: ``x y z nx ny nz red green blue`` per vertex (colours as 8-bit), ``3 i j k`` per face"""
    rgb = np.clip(np.rint(colors[:, :3] * 255.0), 0, 255).astype(np.int64)
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\ncomment lightplane_amd marching cubes\n")
        f.write(f"element vertex {vertices.shape[0]}\n")
        f.write("property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n")
        f.write("property uchar red\nproperty uchar green\nproperty uchar blue\n")
        f.write(f"element face {faces.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n")
        for v, n, c in zip(vertices, normals, rgb):
            f.write(f"{v[0]:.9g} {v[1]:.9g} {v[2]:.9g} {n[0]:.6g} {n[1]:.6g} {n[2]:.6g} {c[0]} {c[1]} {c[2]}\n")
        for t in faces:
            f.write(f"3 {t[0]} {t[1]} {t[2]}\n")


@torch.no_grad()
def pointcloud(renderer, grids, size, threshold, dev):
    """[M, 7] float32 rows ``x y z | r g b | opacity``: the decoder at the lattice points of a size^3 scaffold whose opacity exceeds
    ``threshold``, colours seen along -z"""
    occupied = renderer.calculate_scaffold(grids, [1, size, size, size], dev, threshold=threshold, dilate_scaffold=0)[0]
    lin = torch.linspace(0, 1, size, device=dev) * 2.0 - 1.0
    iz, iy, ix = occupied.nonzero(as_tuple=True)
    xyz = torch.stack([lin[ix], lin[iy], lin[iz]], dim=-1)
    if xyz.shape[0] == 0:
        return torch.zeros(0, 7, device=dev)
    opacity, rgb = renderer.eval_decoder_at_points(xyz[None], torch.zeros(1, dtype=torch.int32, device=dev), None, grids,
                                                   directions=torch.tensor([[0.0, 0.0, -1.0]], device=dev))
    return torch.cat([xyz, rgb[0], opacity[0, :, None]], dim=-1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--stop-transmittance", type=float, default=0.0)
    ap.add_argument("--tv-weight", type=float, default=0.0)
    ap.add_argument("--upsample-steps", type=lambda v: tuple(int(x) for x in v.split(",") if x), default=(),
                    help="comma-separated steps before which the planes are doubled; they start at res / 2^k")
    ap.add_argument("--scaffold-steps", type=lambda v: tuple(int(x) for x in v.split(",") if x), default=(),
                    help="comma-separated steps before which the occupancy scaffold is rebuilt (none: no scaffold)")
    ap.add_argument("--scaffold-size", type=int, default=64, help="points per axis of the scaffold's lattice")
    ap.add_argument("--scaffold-threshold", type=float, default=1e-7, help="opacity above which a lattice point is occupied")
    ap.add_argument("--export-pointcloud", default=None, metavar="FILE.npy",
                    help="after the fit, write xyz | rgb | opacity of the occupied lattice points of a scaffold")
    ap.add_argument("--clip-rays", action="store_true",
                    help="clip every ray batch to the scaffold's occupied span (to the scene box before a scaffold exists)")
    ap.add_argument("--export-mesh", default=None, metavar="FILE.ply",
                    help="after the fit, write the level set of the opacity as a coloured triangle mesh (ASCII PLY)")
    ap.add_argument("--mesh-size", type=int, default=64, help="points per axis of the lattice the mesh is extracted from")
    ap.add_argument("--mesh-level", type=float, default=1.0, help="opacity of the extracted level set")
    ap.add_argument("--res", type=int, default=64, help="resolution of the planes")
    ap.add_argument("--modular", action="store_true",
                    help="render the training batches through ray_samples -> eval_decoder_at_points -> composite_samples")
    ap.add_argument("--importance", type=int, default=0,
                    help="with --modular: new samples per ray drawn from the weights of a coarse pass (importance_samples); 0 = none")
    ap.add_argument("--render-samples", action="store_true",
                    help="with --modular: the fitted march through render_samples (decoder + compositing in one launch at the samples' depths)")
    ap.add_argument("--distortion-weight", type=float, default=0.0,
                    help="with --modular: weight of the distortion loss of the fitted march (distortion_loss); 0 = none")
    a = ap.parse_args(argv)
    assert a.importance == 0 or a.modular, "--importance resamples the modular march: pass --modular as well"
    assert not a.render_samples or a.modular, "--render-samples runs the fitted pass of the modular march: pass --modular as well"
    assert a.distortion_weight == 0.0 or a.modular, "--distortion-weight needs the weights of the modular march: pass --modular as well"
    out = fit(a.steps, a.rays, res=a.res, stop_transmittance=a.stop_transmittance, verbose=True, tv_weight=a.tv_weight,
              upsample_steps=a.upsample_steps, scaffold_steps=a.scaffold_steps, scaffold_size=a.scaffold_size,
              scaffold_threshold=a.scaffold_threshold, export_pointcloud=a.export_pointcloud, clip_rays=a.clip_rays,
              export_mesh=a.export_mesh, mesh_size=a.mesh_size, mesh_level=a.mesh_level, modular=a.modular, importance=a.importance,
              distortion_weight=a.distortion_weight, fused_fine=a.render_samples)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Developer benchmark of the GPU marching cubes (lightplane_amd/mesh.py, csrc/lp_mesh.hip) on one MI355X.

    python scripts/bench_mesh.py [--reps 20] [--warmup 3] [--out profiles/mesh_bench.txt] [--sizes 256,512] [--no-fit] [--trace]
    python scripts/bench_mesh.py --summarize-trace KERNEL_TRACE.csv [--out profiles/mesh_bench.txt]      (no GPU; appends to --out)

Inputs: sphere lattices ``0.6 - |p|`` of 256^3 and 512^3 points at level 0, and the opacity lattice (256^3) of the scene
examples/fit_synthetic_scene.py fits in 150 steps, at level 1.  Per input, device-event windows over --reps calls after --warmup calls:
  count+scan   lp_mesh_count: the count pass, the scan launches and the offsets kernel (one ABI call: an event window cannot split it;
               the per-kernel split comes from a kernel trace -- ``--trace`` runs a few untimed calls for
               ``rocprofv3 --kernel-trace --output-format csv -- python scripts/bench_mesh.py --trace``, and ``--summarize-trace``
               condenses that run's kernel trace into median / min / max per kernel and launch size; durations under the profiler
               run a few per cent longer than in the event windows)
  emit         lp_mesh_emit without and with normals, into exactly sized results
  call         lp.marching_cubes end to end in its default mode (allocation, the host read of the offsets, emit) and in capacity mode
Bytes are what the algorithm has to move, computed from the shapes and the counts (each lattice value and workspace word once per pass
that needs it, the results once), against the nominal 8 TB/s of HBM; they are not hardware counters.  The script needs a GPU.
"""
import argparse
import ctypes
import importlib.util
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import lightplane_amd as lp  # noqa: E402
from lightplane_amd import _lib  # noqa: E402

HBM = 8.0e12  # nominal bytes / s


def windows(fn, reps, warmup):
    """(median, min, max) ms of fn() as device-event windows"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def sphere(n, dev):
    lin = torch.linspace(-1, 1, n, device=dev)
    zz, yy, xx = torch.meshgrid(lin, lin, lin, indexing="ij")
    return (0.6 - torch.sqrt(xx * xx + yy * yy + zz * zz))[None].contiguous()


def fitted_scene(n, dev):
    spec = importlib.util.spec_from_file_location("fit_synthetic_scene", os.path.join(REPO, "examples", "fit_synthetic_scene.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    state = {}

    def grab(renderer, grids):
        state["opacity"] = lp.scaffold_opacity(grids, renderer.get_decoder_params(), [1, n, n, n], gain=renderer.gain,
                                               mask_out_of_bounds_samples=renderer.mask_out_of_bounds_samples)

    out = mod.fit(steps=150, n_rays=4096, on_fitted=grab)
    return state["opacity"], out


def bench(name, vol, level, reps, warmup, say):
    dev = vol.device
    L = _lib.lib()
    stream = _lib.current_stream(dev)
    B, N = vol.shape[0], vol.numel()
    ref = lp.marching_cubes(vol, level, with_normals=True)
    V, F = ref.vertices.shape[0], ref.faces.shape[0]
    a = _lib.LpMeshArgs()
    a.volume, a.shape, a.level = vol.data_ptr(), _lib.LpGrid(*vol.shape, 0, None), float(level)
    ws = torch.empty(lp.mesh_workspace_bytes(vol.shape), dtype=torch.uint8, device=dev)
    vo, fo = torch.empty(B + 1, dtype=torch.int64, device=dev), torch.empty(B + 1, dtype=torch.int64, device=dev)
    a.vertex_offsets, a.face_offsets = vo.data_ptr(), fo.data_ptr()
    verts, faces, normals = torch.empty(V, 3, device=dev), torch.empty(F, 3, dtype=torch.int32, device=dev), torch.empty(V, 3, device=dev)
    a.vertices, a.faces, a.max_vertices, a.max_faces = verts.data_ptr(), faces.data_ptr(), V, F

    def count():
        _lib.check(L.lp_mesh_count(ctypes.byref(a), ws.data_ptr(), ws.numel(), stream), "lp_mesh_count")

    def emit(with_normals):
        a.normals = normals.data_ptr() if with_normals else None
        _lib.check(L.lp_mesh_emit(ctypes.byref(a), ws.data_ptr(), ws.numel(), stream), "lp_mesh_emit")

    tiles = -(-N // 256)
    scan_bytes = 2 * 16 * tiles * (1 + 1 / 256) + 2 * 16 * tiles            # every level read and written once, level 0 once more by the add
    count_bytes = 4 * N + 4 * N + 16 * tiles                                  # lattice in, words and tile sums out
    emit_bytes = 4 * N + 16 * tiles + 12 * V + 12 * F + 8 * V                 # words and tile sums in, results out, two lattice values per vertex
    say(f"\n{name}: {tuple(vol.shape)} = {N} points ({4 * N / 2 ** 20:.0f} MiB), level {level:g}: {V} vertices, {F} faces; "
        f"workspace {ws.numel() / 2 ** 20:.1f} MiB ({ws.numel() / N:.3f} bytes per point)")
    t = windows(count, reps, warmup)
    b = count_bytes + scan_bytes
    say(f"  count+scan        {t[0]:8.3f} ms [{t[1]:.3f} .. {t[2]:.3f}]  {b / 1e6:9.1f} MB -> {b / t[0] / 1e9:7.2f} TB/s = {100 * b / t[0] / 1e-3 / HBM:5.1f} % of 8 TB/s"
        f"   (count {count_bytes / 1e6:.1f} MB, scan {scan_bytes / 1e6:.1f} MB)")
    for wn in (False, True):
        t = windows(lambda: emit(wn), reps, warmup)
        b = emit_bytes + (12 * V if wn else 0)
        say(f"  emit{' + normals' if wn else '          '}    {t[0]:8.3f} ms [{t[1]:.3f} .. {t[2]:.3f}]  {b / 1e6:9.1f} MB -> {b / t[0] / 1e9:7.2f} TB/s = "
            f"{100 * b / t[0] / 1e-3 / HBM:5.1f} % of 8 TB/s")
    assert torch.equal(verts, ref.vertices) and torch.equal(faces, ref.faces) and torch.equal(normals, ref.normals)
    t = windows(lambda: lp.marching_cubes(vol, level), reps, warmup)
    say(f"  call, default     {t[0]:8.3f} ms [{t[1]:.3f} .. {t[2]:.3f}]  (allocates workspace and results; one host read of the offsets)")
    t = windows(lambda: lp.marching_cubes(vol, level, max_vertices=V, max_faces=F, workspace=ws), reps, warmup)
    say(f"  call, capacity    {t[0]:8.3f} ms [{t[1]:.3f} .. {t[2]:.3f}]  (caller workspace; no host synchronisation)")


def summarize_trace(path, say):
    """median / min / max duration per lp::mesh_* kernel and grid size of a rocprofv3 kernel trace (csv)"""
    import csv
    groups = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            if "lp::mesh_" not in name:
                continue
            short = name.split("(")[0].replace("void ", "").replace("lp::", "")
            groups.setdefault((short, int(r["Grid_Size_X"])), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    say("\n# kernel trace (rocprofv3 --kernel-trace, a run of its own: bench_mesh.py --trace, lp.marching_cubes(with_normals=True) five times per "
        "sphere lattice); durations under the profiler, a few per cent above the event windows")
    say("# kernel                 work-items  launches   median us      min      max")
    for (short, grid), us in sorted(groups.items()):
        say(f"  {short:22s} {grid:11d} {len(us):9d} {statistics.median(us):11.1f} {min(us):8.1f} {max(us):8.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarize-trace", default=None, metavar="CSV", help="condense a kernel trace of a --trace run (no GPU needed)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="256,512", help="comma-separated edge lengths of the sphere lattices")
    ap.add_argument("--no-fit", action="store_true", help="skip the fitted scene")
    ap.add_argument("--trace", action="store_true", help="five untimed calls per sphere lattice, for a kernel trace")
    a = ap.parse_args()
    if a.summarize_trace:
        lines = []
        summarize_trace(a.summarize_trace, lambda s: (print(s), lines.append(s)))
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return
    assert torch.cuda.is_available(), "bench_mesh.py measures on a GPU; there is nothing to fall back to"
    dev = torch.device("cuda:0")
    sizes = [int(v) for v in a.sizes.split(",") if v]
    if a.trace:
        for n in sizes:
            vol = sphere(n, dev)
            for _ in range(5):
                lp.marching_cubes(vol, 0.0, with_normals=True)
            torch.cuda.synchronize()
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# mesh bench  {time.strftime('%Y-%m-%d')}  {torch.cuda.get_device_name(0)}  library src {_lib.build_info()['src_hash'][:16]}")
    say(f"# device-event windows, median of {a.reps} calls after {a.warmup} warm-up calls, min / max in brackets; bytes = what the algorithm "
        "has to move (from shapes and counts, not counters), rate against the nominal 8 TB/s")
    for n in sizes:
        bench(f"sphere {n}^3", sphere(n, dev), 0.0, a.reps, a.warmup, say)
        torch.cuda.empty_cache()
    if not a.no_fit:
        vol, fit = fitted_scene(256, dev)
        say(f"\n# fitted scene: examples/fit_synthetic_scene.py, 150 steps of 4096 rays, held-out PSNR {fit['heldout_psnr_db']:.2f} dB")
        bench("fitted scene 256^3", vol, 1.0, a.reps, a.warmup, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

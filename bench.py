#!/usr/bin/env python
"""bench.py -- Mrays/s fwd+bwd of the Lightplane Renderer / Splatter hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload cfg2|cfg4|1080p_s128|cfg3|cfg5|small|refbench|refbench_splatter]
                    [--dump-outputs DIR] [--full [--no-extras] [--no-cpu-baseline]]

Workloads (BASELINE.json `configs`); one step = forward + backward, inputs resident in HBM:
  cfg2        (default, the headline metric) Renderer, 256x256 rays per GPU (pinhole camera looking at the [-1,1]^3
              cube), triplane 3 x 64^2 x 16 ch, 128 samples/ray, trunk/opacity/colour MLPs 2 layers x 32 hidden,
              3 colour channels, 32-wide ray encoding.
  cfg4        Renderer, ONE 1920x1080 camera per GPU (cameras on a ring, elevation 30 deg, azimuth 45 deg x rank),
              triplane 3 x 128^2 x 32 ch, 256 samples -- the 8-GPU ray-shard configuration of BASELINE.json.
  1080p_s128  Renderer, one 1920x1080 camera per GPU on the cfg-2 scene (triplane 64^2 x 16 ch, 128 samples):
              the batch north_star asks the Mrays/s report for.
  cfg3        Splatter, 256x256 rays x 32 ch per GPU -> voxel grid 128^3 x 32 ch, 256 samples.
  cfg5        Joint Splatter -> Renderer (BASELINE configs[4]), weak-scaled: per GPU 13 views of 512x512 rays x 32 ch are
              splatted into a private 256^3 x 32 ch voxel grid, the un-normalised grids + weights are summed over the GPUs
              (reduce-scatter + all-gather: 2.15 GB) and normalised, then every GPU renders its 135 x 1920 rows of a
              1920x1080 camera (x N GPUs) from the replicated grid; end-to-end backward (grid gradient all-reduced, splat
              backward local).  At 8 GPUs: 104 views and one full 1080p frame, as BASELINE names it.
  refbench    the reference's OWN speed benchmark (tests/renderer_speed_benchmark.py:228-285): triplane [3,32,32,32,32]
              (three batch entries, 32^2 planes x 32 ch), hidden 32, 2/2/2 layers, 256 samples, random rays, image sizes
              16 .. 2048 (x sqrt 2 steps); its protocol: fresh inputs per iteration, 2 warm-up + 5 timed reruns, wall time of
              the forward / of the backward bracketed by device synchronisation, peak memory over forward + backward.
  refbench_splatter  tests/splatter_speed_benchmark.py:200-247: 128^2 x num_view random rays x 64 ch -> voxel 160^3 x 64 ch,
              96 samples, mask_out_of_bounds_samples, same protocol.
With N > 1 GPUs (one process per GPU, RCCL) every rank works on its own camera (weak scaling), the grid / parameters
are replicated and the Renderer's grid + MLP gradients (the Splatter's un-normalised output + weight grid) are summed
with an all-reduce INSIDE the timed step.

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times K steps and prints the headline (`value`, `ms_per_step`,
what ran); nothing else touches the GPU.  --dump-outputs DIR then writes what the last timed step computed -- the outputs and
the gradients a caller of the op receives -- as DIR/<name>.npy (see dump_outputs), so that two builds can be compared on the
same seeded inputs.

--full adds everything beyond the headline, measured after the timed steps: `fwd_ms` / `bwd_ms` (HIP events), the
reference-protocol peak memory and `roofline`, for the dominant kernel of the workload (Renderer: the backward
kernel; Splatter: the forward walk): SURVEY.md 8(d)'s algorithmic bytes per launch divided by that kernel's mean
launch time, measured with HIP events on the launch stream (torch's current stream is the stream the C ABI launches on).
At N = 1 with the default workload the --full line also carries `extras`: the other configurations measured the same way
(short runs), so that every number quoted in DESIGN.md / README.md can be recomputed from the driver's BENCH file (at
N > 1 `extras` holds north_star's reporting batches instead: 1920x1080 rays per GPU at S = 128 and the cfg 4 shard,
through the same sharded step with its RCCL all-reduce, bounded by a watchdog), and
`cpu_baseline`: the CPU oracle (oracle/lightplane_oracle.py, the PyTorch restatement of the reference's naive path)
timed on the host cores of rank 0, on BASELINE configs[0] (cfg 1) and on a ray subsample of the benchmarked workload.
"""
import argparse
import glob
import json
import math
import os
import re
import sys
import time

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

import lightplane_amd as lp  # noqa: E402
from lightplane_amd import _lib, parallel  # noqa: E402

HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md: 8 TB/s spec
FP32_PEAK = 157.3e12    # fp32 vector = fp32 MFMA peak
CLOCK_GHZ = 2.4         # MI355X engine clock
N_SIMD = 256 * 4        # 256 CUs x 4 SIMDs
N_SE = 32               # shader engines SQ_BUSY_CYCLES is summed over (8 XCDs x 4)
LOAD_LATENCY_NS = 800.0 # HBM-miss gather latency used for the loads-in-flight estimate (MI355X_MICROARCH.md: ~0.7-0.9 us)
ATOMIC_SEGMENTS_PER_S = 21e9  # 64-byte global_atomic_add_f32 segments the chip retires (scripts/atomics_probe2.hip)
def arithmetic_string(info=None):
    """The record's `arithmetic` field, composed from lp_build_info() of the library that is LOADED (limb counts and matrix
    instructions as compiled), never from a hand-written constant: the string cannot go stale against the kernels (round-5 review)."""
    info = info or _lib.build_info()
    t = info["tuned_bwd"]
    dx = ("gradient operand of the dX chains as two bf16 limbs (2^-17 per value, three of nine limb products)" if t["dx_limbs"] == 2
          else "dX chains three-limb (fp32-equivalent)")
    if "bf16" in t["dw"]:
        dw = ("weight gradients: two-limb bf16 operands on v_mfma_f32_16x16x32_bf16, three limb products (measured on the cfg-2 launch "
              "against fp64 with the kernel's ReLU decisions forced: worst gradient entry 1.05e-5 vs 8.7e-6 with three limbs and fp32 "
              "products, profiles/r05_dx_limbs_ab.txt, r05_dw_bf16_ab.txt)")
    else:
        dw = "weight gradients: fp32 operands on v_mfma_f32_16x16x4_f32"
    return ("tuned family (the headline kernels): forward products -- outputs, the backward's decoder recompute and its ReLU decisions -- "
            "fp32-equivalent bf16x3 (three exact bf16 limbs per fp32 operand, six limb products, fp32 accumulation) on "
            f"v_mfma_f32_32x32x16_bf16; backward: {dx}; {dw}; everything else fp32 VALU.  LpRendererArgs.arithmetic = LP_ARITH_FP32 "
            f"selects per call: {t['arith_fp32']} (the reference's arithmetic; `extras.renderer_cfg2_fp32_arithmetic`).  Other "
            f"families: looped deep {info['loop_bwd_deep']['dw']} / shallow {info['loop_bwd_shallow']['dw']}")


def build_record():
    """What ran: the loaded library's own report (version, source hash, test hooks) and whether it was built from this tree."""
    info = _lib.build_info()
    return {"lib_version": info["version"], "src_hash": info["src_hash"], "built_from_this_tree": _lib.build_matches_tree(),
            "test_hooks": info["test_hooks"], "tuned_bwd": info["tuned_bwd"], "per_file_flags": info["flags"]["per_file"]}


ARITHMETIC = None  # filled by main() from the loaded library (arithmetic_string)
STEP_PROTOCOL = ("forward + backward of the op with the upstream gradients handed to torch.autograd.backward (no loss kernels in the "
                 "timed step; rounds 1-4 timed loss(...).backward(), i.e. + 6 elementwise / reduction kernels: `extras.headline_with_loss_"
                 "kernels` times that protocol once)")


# ----------------------------------------------------------------------------------------------------------------
# workloads
# ----------------------------------------------------------------------------------------------------------------

RENDER_CFGS = {
    #              H     W     S    C   grid  description
    "cfg2": (256, 256, 128, 16, 64, "cfg2: Renderer fwd+bwd, 256x256 rays/GPU, triplane 64^2x16ch, 128 samples, "
                                    "2-layer/32-hidden trunk/opacity/color MLP, 3 colour ch, 32-ch ray encoding"),
    "cfg4": (1080, 1920, 256, 32, 128, "cfg4 shard: Renderer fwd+bwd, 1920x1080 rays/GPU, triplane 128^2x32ch, 256 samples, "
                                       "2-layer/32-hidden MLPs, 3 colour ch, grid replicated + grad all-reduce"),
    "1080p_s128": (1080, 1920, 128, 16, 64, "1080p_s128: Renderer fwd+bwd, 1920x1080 rays/GPU, triplane 64^2x16ch, "
                                            "128 samples, 2-layer/32-hidden MLPs, 3 colour ch"),
    "small": (64, 64, 128, 16, 64, "small batch: Renderer fwd+bwd, 64x64 rays, triplane 64^2x16ch, 128 samples "
                                   "(segment-parallel march, DESIGN.md 4.9)"),
    # hidden width 64: the reference's own example configuration (examples/config/synthetic_overfit.json: triplane 128^2 x 32 ch,
    # mlp_hidden_chn 64, 128 samples; layer counts = the example's defaults 1/1/2, examples/utils/util/config_util.py:165-169)
    "h64_example_112": (256, 256, 128, 32, 128, "hidden 64, the reference example's decoder: Renderer fwd+bwd, 256x256 rays, triplane "
                                                "128^2x32ch, 128 samples, trunk 1 / opacity 1 / colour 2 layers x 64 hidden, 3 colour ch"),
    "h64_222": (256, 256, 128, 32, 128, "hidden 64: Renderer fwd+bwd, 256x256 rays, triplane 128^2x32ch, 128 samples, "
                                        "2-layer/64-hidden trunk/opacity/colour MLPs, 3 colour ch"),
}
RENDER_CFGS["refbench256"] = (256, 256, 256, 32, 32, "refbench256: the 256^2 row of the reference's own speed benchmark (tests/renderer_speed_benchmark.py:228-285) as a "
                                                     "steady-state workload: 65 536 RANDOM rays (tests/utils.py:230-268) over three batch entries, triplane "
                                                     "[3,32,32,32,32], 256 samples, 2/2/2 x 32 decoder with N(0, 0.01) parameters, disparity_at_inf 0.01")
RENDER_CFGS["cfg5_render"] = (135, 1920, 256, 32, 256, "cfg5 render leg alone: Renderer fwd+bwd, 135x1920 rays of a 1080p camera, VOXEL grid 256^3x32ch (2.15 GB: 8x the "
                                                         "Infinity Cache), 256 samples, 2-layer/32-hidden MLPs -- the launch the grid-tile-staging question is about")
VOXEL_CFGS = ("cfg5_render",)
DECODER_SHAPES = {"h64_example_112": ((1, 1, 2), 64), "h64_222": ((2, 2, 2), 64)}  # everything else: 2/2/2 layers x 32 hidden
HIDDEN, COLOR = 32, 3


def camera_pose(name, rank):
    if name == "cfg2":  # rank 0: the axis-aligned view of round 1's headline; other ranks from the ring
        return 45.0 * rank, (0.0 if rank == 0 else 30.0)
    return 45.0 * rank, 30.0  # 8 cameras on a ring, elevation 30 deg


class RendererWorkload:
    def __init__(self, name, rank, dev, pg, kernel, arithmetic=_lib.LP_ARITH_DEFAULT, with_loss=False, march_order=None):
        from tests.synth import grid_sizes_for, pinhole_rays, random_decoder, random_grids

        self.name, self.pg, self.kernel, self.arithmetic, self.with_loss = name, pg, kernel, arithmetic, with_loss
        H, W, S, C, G, self.desc = RENDER_CFGS[name]
        self.S, self.C = S, C
        gen = torch.Generator().manual_seed(0)
        random = name == "refbench256"  # incoherent rays, the reference benchmark's inputs
        self.sizes = grid_sizes_for((3 if random else 1, G, G, G, C), name not in VOXEL_CFGS)
        if name in VOXEL_CFGS:  # (2.15 GB: drawn on the device, in slices)
            self.grids_c = None
        else:
            self.grids_c = random_grids(gen, self.sizes)
        self.layers, self.hidden = DECODER_SHAPES.get(name, ((2, 2, 2), HIDDEN))
        self.dec_c = random_decoder(gen, *self.layers, C, self.hidden, COLOR, std=0.01 if random else 0.15 if self.hidden == 32 else 0.1)
        gen_r = torch.Generator().manual_seed(100 + rank)
        az, el = camera_pose(name, rank)
        if random:
            from tests.synth import random_rays
            self.rays_c = random_rays(gen_r, H * W, 3, int(self.dec_c.n_hidden_color[0]))
        else:
            self.rays_c = pinhole_rays(H, W, enc_dim=int(self.dec_c.n_hidden_color[0]), gen=gen_r, azimuth_deg=az, elevation_deg=el)
        # (bench.py runs with check_inputs off -- no device sync in a timed step --, so "auto" cannot look at the rays: the random-ray
        # workload names its march order; LP_BENCH_MARCH=rays for the A/B)
        self.render_kw = dict(disparity_at_inf=0.01, march_order=march_order or os.environ.get("LP_BENCH_MARCH", "samples")) if random else {}

        n = H * W
        up = (torch.randn(n, generator=gen_r), torch.randn(n, generator=gen_r), torch.randn(n, COLOR, generator=gen_r))
        self.n_rays = n
        self.rays = self.rays_c.to(dev)
        if self.grids_c is None:
            gd = torch.Generator(device=dev).manual_seed(0)
            self.flat = torch.empty(G * G * G, C, device=dev)
            for z in range(0, G * G * G, 1 << 22):
                self.flat[z:z + (1 << 22)] = torch.randn(min(1 << 22, G * G * G - z), C, device=dev, generator=gd)
        else:
            self.flat, _ = lp.flatten_grid([g.to(dev) for g in self.grids_c])
        self.flat.requires_grad_(True)
        self.params = self.dec_c.mlp_params.to(dev).requires_grad_(True)
        self.rays.encoding.requires_grad_(True)
        self.dec = lp.DecoderParams(self.params, self.dec_c.n_hidden_trunk, self.dec_c.n_hidden_opacity,
                                    self.dec_c.n_hidden_color, COLOR)
        self.up = [u.to(dev) for u in up]

    # bytes/ray = S*K*C*4 gathered (fwd) ; the same re-gathered + the same as atomic payload (bwd) ; + ray I/O
    def algorithmic_bytes(self):
        per_sample = (8 if self.name in VOXEL_CFGS else 12) * self.C * 4  # triplane: 3 planes x 4 corners; voxel grid: 8 corners
        return self.n_rays * (self.S * per_sample + 184), self.n_rays * (self.S * per_sample * 2 + 316)

    def mlp_flops_fwdbwd(self):
        dims = [[int(v) for v in x] for x in (self.dec_c.n_hidden_trunk, self.dec_c.n_hidden_opacity, self.dec_c.n_hidden_color)]
        dims[2][-1] = COLOR  # (the colour output layer is padded in the parameter vector; count the real channels)
        mac = sum(a * b for x in dims for a, b in zip(x[:-1], x[1:]))
        return 2 * mac * self.S * 4 * self.n_rays  # forward + (recompute + dX + dW)

    def dw_f32_mfma_per_launch(self):
        """v_mfma_f32_16x16x4_f32 of the weight-gradient quadrants per backward launch, from the decoder's REAL layer list:
        32 rays x (in x out) MACs of every layer that feeds a hidden activation (all trunk layers, every head layer but its
        output layer, which runs on the VALU) / 1 024 MACs per instruction, per wave-sample (2/2/2 x 32: C=16 112, C=32 128;
        2/2/2 x 64 on C=32: 448).  None when the layer list cannot be read (the caller then falls back to a ratio)."""
        try:
            t, o, c = ([int(v) for v in x] for x in (self.dec_c.n_hidden_trunk, self.dec_c.n_hidden_opacity, self.dec_c.n_hidden_color))
            pad = lambda v: -(-v // 16) * 16  # noqa: E731  (operand tiles are 16 wide)
            macs = sum(pad(a) * pad(b) for a, b in zip(t[:-1], t[1:]))
            macs += sum(pad(a) * pad(b) for x in (o, c) for a, b in zip(x[:-2], x[1:-1]))
            return (self.n_rays // 32) * self.S * (macs // 32)
        except Exception:
            return None

    def zero_grads(self):
        self.flat.grad = self.params.grad = self.rays.encoding.grad = None

    def forward(self, replicated=True):
        g, p = (self.flat, self.params)
        if replicated:
            g, p = parallel.replicate_with_grad_allreduce([self.flat, self.params], self.pg)
        d = lp.DecoderParams(p, self.dec.n_hidden_trunk, self.dec.n_hidden_opacity, self.dec.n_hidden_color, COLOR)
        return lp.lightplane_renderer(self.rays, g, d, num_samples=self.S, gain=1.0, grid_sizes=self.sizes, kernel=self.kernel,
                                      arithmetic=self.arithmetic, **self.render_kw)

    def loss(self, out):
        return (out[0] * self.up[0]).sum() + (out[1] * self.up[1]).sum() + (out[2] * self.up[2]).sum()

    def step(self):
        # one step = forward + backward of the op; the upstream gradients are handed to the backward directly (no loss kernels in
        # the timed region: they are the harness's, not the hot path's)
        self.zero_grads()
        out = self.forward()
        if self.with_loss:  # the protocol of rounds 1-4 (and of the reference's benchmark): a scalar loss and its backward
            self.loss(out).backward()
        else:
            torch.autograd.backward(list(out[:3]), self.up)
        return out

    def results(self, out):
        """What a caller of the step receives: the op's outputs and the gradients of its inputs."""
        return {"ray_length": out[0], "neg_log_t": out[1], "feature": out[2], "grad_grid": self.flat.grad,
                "grad_mlp_params": self.params.grad, "grad_encoding": self.rays.encoding.grad}

    roofline_kernel = "renderer backward"

    def roofline(self, fwd_ms, bwd_ms):
        fwd_b, bwd_b = self.algorithmic_bytes()
        ach = bwd_b / (bwd_ms * 1e-3) / 1e9
        both = (fwd_b + bwd_b) / ((fwd_ms + bwd_ms) * 1e-3) / 1e9
        return {"bound": "hbm", "kernel": self.roofline_kernel, "achieved": round(ach, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(ach / HBM_PEAK_GBS, 5), "algorithmic_bytes_per_launch": bwd_b,
                "frac_fwd_plus_bwd": round(both / HBM_PEAK_GBS, 5)}


class SplatterWorkload:
    """cfg 3: 256x256 rays x 32 ch -> voxel 128^3 x 32 ch, S = 256 (atomic scatter-add path)."""

    name = "cfg3"
    desc = "cfg3: Splatter fwd+bwd, 256x256 rays/GPU x 32ch encoding -> 128^3x32ch voxel grid, 256 samples"
    roofline_kernel = "splatter forward walk"

    def __init__(self, rank, dev, pg, image=(256, 256)):
        from tests.synth import pinhole_rays

        self.pg, self.S, self.C, self.G = pg, 256, 32, 128
        self.row = None if os.environ.get("LP_BENCH_NO_ROW_HINT") else image[1]  # rays per image row (detected by the front-end when check_inputs is on)
        gen = torch.Generator().manual_seed(100 + rank)
        az, el = camera_pose("cfg2", rank)
        self.rays_c = pinhole_rays(image[0], image[1], gen=gen, azimuth_deg=az, elevation_deg=el)
        self.rays_c.encoding = torch.rand(self.rays_c.n_rays, self.C, generator=gen)
        self.rays = self.rays_c.to(dev)
        self.rays.encoding.requires_grad_(True)
        self.n_rays = self.rays.n_rays
        self.sizes = [[1, self.G, self.G, self.G, self.C]]
        self.up = torch.randn(self.G ** 3, self.C, generator=gen).to(dev)

    # S*(K*C*4 + K*4) atomics forward, S*K*C*4 gathered backward (K = 8 corners)
    def algorithmic_bytes(self):
        return self.n_rays * self.S * (8 * self.C * 4 + 8 * 4), self.n_rays * self.S * 8 * self.C * 4

    def zero_grads(self):
        self.rays.encoding.grad = None

    def forward(self, replicated=True):
        return lp.lightplane_splatter(self.rays, self.sizes, num_samples=self.S, return_list=False,
                                      process_group=self.pg if replicated else None, rays_per_row=self.row)

    def loss(self, out):
        return (out * self.up).sum()

    def step(self):
        self.zero_grads()
        out = self.forward()
        torch.autograd.backward([out], [self.up])  # upstream gradient handed over directly (no loss kernels)
        return out

    def results(self, out):
        return {"splat_grid": out, "grad_encoding": self.rays.encoding.grad}

    def roofline(self, fwd_ms, bwd_ms):
        fwd_b, bwd_b = self.algorithmic_bytes()
        ach = fwd_b / (fwd_ms * 1e-3) / 1e9
        both = (fwd_b + bwd_b) / ((fwd_ms + bwd_ms) * 1e-3) / 1e9
        return {"bound": "hbm", "kernel": self.roofline_kernel, "achieved": round(ach, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(ach / HBM_PEAK_GBS, 5), "algorithmic_bytes_per_launch": fwd_b,
                "frac_fwd_plus_bwd": round(both / HBM_PEAK_GBS, 5),
                "note": "fwd = splat walk + normalise + torch zero-fill of the 268 MB grid; SURVEY 8(d)'s 532 936 B/ray"}



# ----------------------------------------------------------------------------------------------------------------
# the reference's own speed benchmarks (its published axes)
# ----------------------------------------------------------------------------------------------------------------
REFBENCH_SIZES = [16, 16 * math.sqrt(2), 32, 32 * math.sqrt(2), 64, 64 * math.sqrt(2), 128, 128 * math.sqrt(2), 256,
                  256 * math.sqrt(2), 512, 512 * math.sqrt(2), 1024, 1024 * math.sqrt(2), 2048]
REFBENCH_VIEWS = [1, 2, 4, 8, 16, 32, 64, 128, 256]


def _ref_protocol(make_inputs, run, dev, n_reruns=5, n_warmup=2):
    """tests/renderer_speed_benchmark.py:108-186 / tests/utils.py:33-77: per iteration fresh (re-seeded) inputs; forward timed
    with wall clock between two device synchronisations; a second forward (untimed) + backward timed the same way; peak memory
    of forward / of forward + backward over the inputs-only base; averages over the reruns after the warm-up."""
    rec = []
    for it in range(n_reruns + n_warmup):
        inp = make_inputs(it)
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        t0 = time.time()
        out = run(inp)
        torch.cuda.synchronize(dev)
        t_fw = time.time() - t0
        mem_fw = (torch.cuda.max_memory_allocated(dev) - base) / 1024.0 / 1000.0  # the reference's "MB"
        del out, inp
        inp = make_inputs(it)
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        out = run(inp)
        outs = out if isinstance(out, (tuple, list)) else (out,)
        grad_var = sum((o * torch.randn_like(o)).mean() for o in outs)
        torch.cuda.synchronize(dev)
        t0 = time.time()
        grad_var.backward()
        torch.cuda.synchronize(dev)
        t_bw = time.time() - t0
        mem_bw = (torch.cuda.max_memory_allocated(dev) - base) / 1024.0 / 1000.0
        del out, outs, grad_var, inp
        if it >= n_warmup:
            rec.append((t_fw, t_bw, mem_fw, mem_bw))
    n = len(rec)
    res = {"t_fw_kernel_ms": round(sum(r[0] for r in rec) / n * 1e3, 4), "t_bw_kernel_ms": round(sum(r[1] for r in rec) / n * 1e3, 4),
           "max_mem_fw_kernel_mb": round(sum(r[2] for r in rec) / n, 3), "max_mem_bw_kernel_mb": round(sum(r[3] for r in rec) / n, 3)}
    # Beside the reference's wall-clock protocol (which, at small sizes, measures the allocator and the host side of a call --
    # e.g. the 1.05 GB zero-fill of the Splatter's output grid -- not the kernels): device time of this package's kernels in one
    # more forward + backward, from torch.profiler's device timeline.
    from torch.profiler import ProfilerActivity, profile
    inp = make_inputs(0)
    torch.cuda.synchronize(dev)
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = run(inp)
        outs = out if isinstance(out, (tuple, list)) else (out,)
        sum((o * torch.randn_like(o)).mean() for o in outs).backward()
        torch.cuda.synchronize(dev)
    fw = bw = other = 0.0
    for e in prof.events():
        if e.device_type != torch.autograd.DeviceType.CUDA:
            continue
        if "lp::" in e.name:
            if "_bwd" in e.name or "backward" in e.name:
                bw += e.device_time_total
            else:
                fw += e.device_time_total
        else:
            other += e.device_time_total
    res.update(lp_kernels_fw_device_ms=round(fw / 1e3, 4), lp_kernels_bw_device_ms=round(bw / 1e3, 4),
               torch_kernels_device_ms=round(other / 1e3, 4))
    del out, outs, inp
    return res


def _device_random_rays(gen, n, batch, enc_dim, dev):
    """tests/utils.py:230-268 of the reference: its benchmark draws the rays ON the device (torch.randn(..., device=device)); so does
    this (a CPU draw + copy leaves the GPU idle for milliseconds between the protocol's synchronisations)."""
    rn = lambda *shape: torch.randn(*shape, device=dev, generator=gen)  # noqa: E731
    grid_idx = torch.randint(0, batch, (n,), device=dev, generator=gen, dtype=torch.long)
    origins = rn(n, 3) / 3.0
    directions = -origins + rn(n, 3) * 0.1
    near = rn(n) * 0.1 + 0.1
    far = rn(n).abs() * 0.1 + 3.0
    enc = None if enc_dim is None else rn(n, enc_dim)
    return lp.Rays(directions=directions, origins=origins, grid_idx=grid_idx, near=near, far=far, encoding=enc)


def refbench_renderer(dev, sizes=None, kernel=_lib.LP_KERNEL_AUTO, n_reruns=5, n_warmup=2):
    """tests/renderer_speed_benchmark.py:228-285 on this implementation: grid [3,32,32,32,32] as a triplane (three batch entries),
    2/2/2 x 32 decoder with N(0, 0.01) parameters (tests/utils.py:349), 256 samples, random rays (tests/utils.py:230-268)."""
    from tests.synth import grid_sizes_for, random_decoder, random_grids, random_rays
    rows = []
    for im in (sizes or REFBENCH_SIZES):
        n = int(im ** 2)

        def make_inputs(it):
            gen = torch.Generator().manual_seed(it)
            gsz = grid_sizes_for((3, 32, 32, 32, 32), True)
            grids = [g.to(dev).requires_grad_(True) for g in random_grids(gen, gsz)]
            dec = random_decoder(gen, 2, 2, 2, 32, 32, 3, std=0.01)
            params = dec.mlp_params.to(dev).requires_grad_(True)
            rays = _device_random_rays(torch.Generator(device=dev).manual_seed(it), n, 3, 32, dev)
            rays.encoding.requires_grad_(True)
            return rays, grids, lp.DecoderParams(params, dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, 3)

        def run(inp):
            rays, grids, dec = inp
            return lp.lightplane_renderer(rays, grids, dec, num_samples=256, gain=1.0, disparity_at_inf=0.01, inject_noise_seed=0,
                                          kernel=kernel)

        # the reference's call path checks grid_idx on the host (lightplane_renderer.py:464-467: a device sync per call); with it on,
        # march_order "auto" sees that these rays are unrelated and marches samples per wavefront (no extra sync)
        saved = lp.config.check_inputs
        lp.config.check_inputs = True
        try:
            r = _ref_protocol(make_inputs, run, dev, n_reruns, n_warmup)
        finally:
            lp.config.check_inputs = saved
        r.update(num_rays=n, image_size=int(n ** 0.5),
                 Mrays_per_s_fwd_bwd=round(n / (r["t_fw_kernel_ms"] + r["t_bw_kernel_ms"]) / 1e3, 4))
        rows.append(r)
    return {"benchmark": "reference tests/renderer_speed_benchmark.py:228-285: triplane [3,32,32,32,32], hidden 32, 2/2/2 layers, S=256, "
                         f"random rays; wall time incl. host side and output / gradient allocation, {n_warmup} warm-up + {n_reruns} reruns",
            "published_reference": "SURVEY 6: 256^2 rays fwd ~28 ms / bwd ~0.32 s (figure in the reference's README, A100-class GPU, Triton)",
            "rows": rows}


def refbench_splatter(dev, views=None, n_reruns=5, n_warmup=2):
    """tests/splatter_speed_benchmark.py:200-247: 128^2 x num_view random rays x 64 ch -> voxel [1,160,160,160,64], S = 96,
    mask_out_of_bounds_samples."""
    from tests.synth import random_rays
    rows = []
    sizes = [[1, 160, 160, 160, 64]]
    for nv in (views or REFBENCH_VIEWS):
        n = 128 * 128 * nv

        def make_inputs(it):
            gen = torch.Generator(device=dev).manual_seed(it)
            rays = _device_random_rays(gen, n, 1, None, dev)
            rays.encoding = torch.rand(n, 64, device=dev, generator=gen)
            rays.encoding.requires_grad_(True)
            return rays

        def run(rays):
            return lp.lightplane_splatter(rays, sizes, num_samples=96, mask_out_of_bounds_samples=True)

        saved = lp.config.check_inputs  # (the reference's call path checks grid_idx with a device sync; "auto" march order rides on it)
        lp.config.check_inputs = True
        try:
            r = _ref_protocol(make_inputs, run, dev, n_reruns, n_warmup)
        finally:
            lp.config.check_inputs = saved
        r.update(num_view=nv, num_rays=n, Mrays_per_s_fwd_bwd=round(n / (r["t_fw_kernel_ms"] + r["t_bw_kernel_ms"]) / 1e3, 4))
        rows.append(r)
    return {"benchmark": "reference tests/splatter_speed_benchmark.py:200-247: 128^2 x num_view random rays x 64 ch -> voxel "
                         f"[1,160,160,160,64] (1.05 GB), S=96, mask_out_of_bounds_samples; wall time, {n_warmup} warm-up + {n_reruns} reruns",
            "rows": rows}


class JointWorkload:
    """cfg 5 (BASELINE configs[4]), weak-scaled per GPU: splat V views -> sum over GPUs -> normalise -> render this GPU's rows of
    a 1920x1080 camera from the replicated grid -> end-to-end backward.  Sizes from the environment for the two-rank test
    (CFG5_VIEWS, CFG5_IMG, CFG5_GRID, CFG5_ROWS, CFG5_S)."""

    name = "cfg5"
    roofline_kernel = "splatter forward walk"

    def __init__(self, rank, world, dev, pg, kernel):
        from tests.synth import pinhole_rays, random_decoder
        env = lambda k, d: int(os.environ.get(k, d))  # noqa: E731
        self.pg, self.kernel = pg, kernel
        self.V, self.img, self.G, self.rows, self.S, self.C = env("CFG5_VIEWS", 13), env("CFG5_IMG", 512), env("CFG5_GRID", 256), \
            env("CFG5_ROWS", 135), env("CFG5_S", 256), 32
        gen = torch.Generator().manual_seed(1000 + rank)
        tot = self.V * max(world, 1)
        parts = []
        for v in range(self.V):
            k = rank * self.V + v
            r = pinhole_rays(self.img, self.img, gen=gen, azimuth_deg=360.0 * k / tot, elevation_deg=40.0 * math.sin(2 * math.pi * k / tot))
            parts.append(r)
        from tests.synth import cat_rays
        rays = cat_rays(parts)
        rays.encoding = torch.rand(rays.n_rays, self.C, generator=gen)
        self.splat_rays = rays.to(dev)
        self.splat_rays.encoding.requires_grad_(True)
        H, W = 1080, 1920
        cam = pinhole_rays(H, W, enc_dim=32, gen=torch.Generator().manual_seed(5))
        r0 = (rank * self.rows) % (H - self.rows + 1)
        self.cam = cam[r0 * W:(r0 + self.rows) * W].to(dev)
        dec_c = random_decoder(torch.Generator().manual_seed(0), 2, 2, 2, self.C, 32, 3, std=0.15)
        self.params = dec_c.mlp_params.to(dev).requires_grad_(True)
        self.dec_c = dec_c
        self.sizes = [[1, self.G, self.G, self.G, self.C]]
        self.n_rays = self.splat_rays.n_rays + self.cam.n_rays
        self.desc = (f"cfg5 per GPU: {self.V} views {self.img}x{self.img} x32ch -> {self.G}^3x32ch voxel (sum over GPUs by reduce-scatter + "
                     f"all-gather, then normalise), render {self.rows}x1920 rays of a 1080p camera at {self.S} samples, end-to-end backward")

    def zero_grads(self):
        self.params.grad = self.splat_rays.encoding.grad = None

    def forward(self, replicated=True):
        pg = self.pg if replicated else None
        row = not os.environ.get("LP_BENCH_NO_ROW_HINT")
        grid = lp.lightplane_splatter(self.splat_rays, self.sizes, num_samples=self.S, return_list=False, process_group=pg,
                                      rays_per_row=self.img if row else None)
        p = self.params
        if replicated:  # the splatted grid is a replicated tensor consumed by ray shards: its gradient is summed over the GPUs
            grid, p = parallel.replicate_with_grad_allreduce([grid, self.params], self.pg, exclusive_grads=True)  # consumed by the Renderer only
        d = lp.DecoderParams(p, self.dec_c.n_hidden_trunk, self.dec_c.n_hidden_opacity, self.dec_c.n_hidden_color, 3)
        return lp.lightplane_renderer(self.cam, grid, d, num_samples=self.S, gain=1.0, grid_sizes=self.sizes, kernel=self.kernel)

    def loss(self, out):
        return out[0].sum() + out[1].sum() + out[2].sum()

    def step(self):
        self.zero_grads()
        out = self.forward()
        self.loss(out).backward()
        return out

    def results(self, out):
        return {"ray_length": out[0], "neg_log_t": out[1], "feature": out[2], "grad_mlp_params": self.params.grad,
                "grad_splat_encoding": self.splat_rays.encoding.grad}

    def roofline(self, fwd_ms, bwd_ms):
        ns, nr, S, C = self.splat_rays.n_rays, self.cam.n_rays, self.S, self.C
        b = ns * S * (8 * C * 4 + 8 * 4) + ns * S * 8 * C * 4 + nr * (S * 8 * C * 4 * 3 + 500)
        ach = b / ((fwd_ms + bwd_ms) * 1e-3) / 1e9
        return {"bound": "hbm", "kernel": "whole step (splat fwd+bwd, render fwd+bwd)", "achieved": round(ach, 2), "peak": HBM_PEAK_GBS,
                "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 5), "algorithmic_bytes_per_launch": b, "frac_fwd_plus_bwd": round(ach / HBM_PEAK_GBS, 5)}


def make_workload(name, rank, dev, pg, kernel, **kw):
    if name == "cfg3":
        return SplatterWorkload(rank, dev, pg)
    if name == "cfg5":
        return JointWorkload(rank, int(os.environ.get("WORLD_SIZE", "1")), dev, pg, kernel)
    return RendererWorkload(name, rank, dev, pg, kernel, **kw)


def event_times(wl, reps):
    """Mean forward / backward time of the op itself (no collective): HIP events on the launch stream, the host runs
    ahead of the GPU so the events bracket the kernels back to back (the first two iterations fill the queue)."""
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(reps + 2)]
    for ev in evs:
        wl.zero_grads()
        ev[0].record()
        out = wl.forward(replicated=False)
        ev[1].record()
        loss = wl.loss(out)
        ev[2].record()
        loss.backward()
        ev[3].record()
    torch.cuda.synchronize()
    fwd_ms = sum(ev[0].elapsed_time(ev[1]) for ev in evs[2:]) / reps
    bwd_ms = sum(ev[2].elapsed_time(ev[3]) for ev in evs[2:]) / reps
    return fwd_ms, bwd_ms


_PMC_FILE = re.compile(r"r(\d+)_pmc_summary\.json$")  # the per-round summaries of the DEFAULT command; r03loop_* etc. are experiments


def observed_kernels(wl, reps=3):
    """Names and mean device time (ms per launch) of the lp:: kernels ONE step of this workload launches, from
    torch.profiler's device timeline -- so that committed counters are looked up by the kernel that ran here."""
    from torch.profiler import ProfilerActivity, profile

    def local_step():  # no collective: only rank 0 runs this pass
        wl.zero_grads()
        wl.loss(wl.forward(replicated=False)).backward()

    local_step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            local_step()
        torch.cuda.synchronize()
    acc = {}
    for e in prof.events():
        if e.device_type != torch.autograd.DeviceType.CUDA or "lp::" not in e.name:
            continue
        acc.setdefault(e.name.split("(")[0].replace("void ", "").strip(), []).append(e.device_time_total)
    return {k: {"launches_per_step": len(v) / reps, "mean_ms": sum(v) / len(v) / 1e3} for k, v in acc.items()}


def dominant_kernel(observed, substr):
    """The observed kernel whose name contains `substr` with the largest device time per step (None if none ran)."""
    best = None
    for k, v in (observed or {}).items():
        if substr in k and (best is None or v["mean_ms"] * v["launches_per_step"] > best[1]):
            best = (k, v["mean_ms"] * v["launches_per_step"])
    return best[0] if best else None


def pmc_entry(workload, kernel_name, profiles_dir=None):
    """Per-launch counter averages of `kernel_name` (the EXACT instantiation that ran, e.g.
    "lp::renderer_bwd_bf3<16, 1, true, 3, 4, false>") from the committed rocprofv3 PMC passes of the default command
    (profiles/rNN_pmc_summary.json, newest round first; separate --pmc runs of `bench.py --workload <w>`,
    scripts/gpu_profile.sh).  NOT measured in this run.  Never falls back to another kernel's counters."""
    if not kernel_name:
        return None, None, None
    d0 = profiles_dir or os.path.join(REPO, "profiles")
    files = [f for f in glob.glob(os.path.join(d0, "r*_pmc_summary.json")) if _PMC_FILE.search(os.path.basename(f))]
    files.sort(key=lambda f: int(_PMC_FILE.search(os.path.basename(f)).group(1)), reverse=True)
    want = kernel_name.replace(" ", "")
    for f in files:
        try:
            d = json.load(open(f))
        except Exception:
            continue
        for k, v in d.items():
            if ": " not in k or not isinstance(v, dict):
                continue
            if k.startswith(workload + ": ") and k.split(": ", 1)[1].replace(" ", "") == want and "hbm_bytes_per_launch" in v:
                return v, os.path.relpath(f, REPO), k.split(": ", 1)[1]
    return None, None, None


def pmc_traffic(workload, kernel_name):
    v, src, _ = pmc_entry(workload, kernel_name)
    return (int(v["hbm_bytes_per_launch"]), src) if v else (None, None)


def counter_clock_ghz(v):
    """Shader clock during the counter pass: SQ_BUSY_CYCLES is summed over the 32 shader engines, the pass's own kernel
    duration is recorded next to it (scripts/summarize_profiles.py).  None when the summary predates that field."""
    busy, dur = v.get("SQ_BUSY_CYCLES"), v.get("pmc_duration_ns") or v.get("trace_duration_ns")
    if not busy or not dur:
        return None
    return busy / N_SE / dur


def issue_bound(v, kname, dw_f32_mfma=None):
    """Issue cycles per SIMD of one launch from its instruction counts (see binding_ceiling)."""
    valu, mfma = v["SQ_INSTS_VALU"], v["SQ_INSTS_MFMA"]
    if "renderer_bwd_bf3_tm" in kname:  # transposed march: bf16 pipe only (two-limb dX, bf16 dW quadrants)
        return valu * 4.0 / N_SIMD
    if "renderer_bwd_bf3" in kname and kname.count(",") >= 6:
        # the tuned backward since round 5 (<C, GM, PLAIN, NC, NW, SEG, DUMP, F32>): its weight-gradient products run on the bf16 pipe
        # too (v_mfma_f32_16x16x32_bf16) -- no MFMA serialises with the VALU any more -- unless it is an LP_ARITH_FP32 instantiation
        # (last argument true: fp32 quadrants, v_mfma_f32_16x16x4_f32, 32 cycles each on top of the VALU)
        args = [x.strip() for x in kname[kname.index("<") + 1: kname.rindex(">")].split(",")] if "<" in kname and ">" in kname else []
        if len(args) >= 8 and args[7] == "true":
            f32 = min(dw_f32_mfma, mfma) if dw_f32_mfma else mfma * 112.0 / 292.0
            return (valu * 4.0 + f32 * 32.0) / N_SIMD
        return valu * 4.0 / N_SIMD
    if "renderer_bwd_loop" in kname:
        # layer-looped backward <C, NB, TG, MT, MH, WC, GM>: the two-waves-per-SIMD shallow instantiations (NB = 1, MT <= 2, MH <= 1, no
        # wide colour) keep fp32 weight-gradient quadrants; every other (one-wave) instantiation has them on the bf16 pipe since round 5
        m = re.search(r"<\s*(\d+),\s*(\d+),\s*(\w+),\s*(\d+),\s*(\d+),\s*(\w+)", kname)
        shallow = bool(m) and int(m.group(2)) == 1 and int(m.group(4)) <= 2 and int(m.group(5)) <= 1 and m.group(6) == "false"
        if m and not shallow:
            return valu * 4.0 / N_SIMD
    if "bf3" in kname or "_loop" in kname:  # bf16x3 families: only the fp32 16x16x4 dW MFMAs serialise with the VALU
        f32 = min(dw_f32_mfma, mfma) if dw_f32_mfma else mfma * 112.0 / 202.0
        return (valu * 4.0 + f32 * 32.0) / N_SIMD
    # fp32-MFMA kernels: every MFMA adds (32x32x2: 64 cycles, 16x16x4: 32 cycles; 120 : 112 per wave-sample)
    return (valu * 4.0 + mfma * (120.0 * 64.0 + 112.0 * 32.0) / 232.0) / N_SIMD


def binding_ceiling(workload, wl, fwd_ms, bwd_ms, observed=None):
    """The ceiling that actually binds the dominant kernel, next to the nominal HBM line (whose algorithmic bytes are served
    by the L2 and by run-merging in registers: fractions above 1 are possible there and say nothing about a hardware limit).

    Renderer backward: INSTRUCTION ISSUE.  A SIMD issues one wave64 VALU instruction per 4 cycles, and fp32
    v_mfma_f32_16x16x4_f32 (the weight-gradient quadrants of the looped family, and of the tuned family until round 4; 32 cycles
    each) do not overlap with VALU work (profiles/r02_mfma_valu_overlap.txt), while the bf16 MFMAs do.  bound = (VALU x 4 +
    fp32-MFMA x 32) cycles per SIMD / clock (tuned family since round 5: VALU x 4 -- every product is on the bf16 pipe); frac_issue = bound / measured time (1.0 = nothing but issue; the rest is waits: barriers, LDS, memory).
    The clock is the one the counters saw (SQ_BUSY_CYCLES / 32 SEs / duration), not the nominal 2.4 GHz.
    Splatter forward: ATOMIC SEGMENTS.  frac_segments = 64-byte atomic segments per launch (WRITE_SIZE / 64 B) / time / 21 G/s.
    Splatter backward walk: issue bound as above + the loads in flight its latency-bound gather sustains.
    Instruction and segment counts come from the committed PMC passes of the SAME kernel instantiation that ran here (looked
    up by exact name), not from this run; when that instantiation has no committed counters the block is null."""
    renderer = isinstance(wl, RendererWorkload)
    kname = dominant_kernel(observed, "renderer_bwd" if renderer else "splat_fwd_walk")
    v, src, kname = pmc_entry(workload, kname)
    if v is None:
        return None
    if renderer:
        if not v.get("SQ_INSTS_VALU") or not v.get("SQ_INSTS_MFMA"):
            return None
        cyc = issue_bound(v, kname, wl.dw_f32_mfma_per_launch())
        clk = counter_clock_ghz(v)
        bound_ms = cyc / ((clk or CLOCK_GHZ) * 1e6)
        t_ms = bwd_ms  # HIP events around the backward (the profiler pass only names the kernel; its own timings run ~10 % long)
        return {"kind": "issue", "kernel": kname, "valu_insts_per_launch": v["SQ_INSTS_VALU"], "mfma_insts_per_launch": v["SQ_INSTS_MFMA"],
                "issue_cycles_per_simd": round(cyc), "clock_ghz": round(clk or CLOCK_GHZ, 3),
                "clock_source": "SQ_BUSY_CYCLES / 32 SEs / kernel duration of the counter pass" if clk else "nominal (summary has no duration)",
                "bound_ms": round(bound_ms, 4), "kernel_ms": round(t_ms, 4),
                "frac_issue": round(bound_ms / t_ms, 4), "source": src + " (committed counter passes, not this run)"}
    w = v.get("WRITE_SIZE")
    if not w:
        return None
    segs = w * 1024.0 / 64.0
    t_ms = observed[kname]["mean_ms"] if observed and kname in observed else fwd_ms
    out = {"kind": "atomic segments", "kernel": kname, "segments_per_launch": round(segs), "peak_segments_per_s": ATOMIC_SEGMENTS_PER_S,
           "kernel_ms": round(t_ms, 4),
           "achieved_segments_per_s": round(segs / (t_ms * 1e-3)), "frac_segments": round(segs / (t_ms * 1e-3) / ATOMIC_SEGMENTS_PER_S, 4),
           "source": src + " (committed counter passes, not this run)"}
    # the backward walk: a latency-bound gather -- issue bound and loads in flight
    kb = dominant_kernel(observed, "splat_bwd_walk")
    vb, srcb, kb = pmc_entry(workload, kb)
    if vb and vb.get("SQ_INSTS_VALU"):
        clk = counter_clock_ghz(vb)
        cyc = vb["SQ_INSTS_VALU"] * 4.0 / N_SIMD
        bms = cyc / ((clk or CLOCK_GHZ) * 1e6)
        tb = observed[kb]["mean_ms"] if observed and kb in observed else bwd_ms
        vm = vb.get("SQ_INSTS_VMEM")
        out["backward"] = {"kind": "issue + loads in flight", "kernel": kb, "valu_insts_per_launch": vb["SQ_INSTS_VALU"],
                           "clock_ghz": round(clk or CLOCK_GHZ, 3), "bound_ms": round(bms, 4), "kernel_ms": round(tb, 4),
                           "frac_issue": round(bms / tb, 4),
                           "vmem_insts_per_launch": vm,
                           "wave_loads_in_flight_per_simd": (round(vm * LOAD_LATENCY_NS * 1e-6 / tb / N_SIMD, 2) if vm else None),
                           "note": f"loads in flight = wave-level VMEM instructions x {LOAD_LATENCY_NS:.0f} ns (L2-miss gather latency, "
                                   "MI355X_MICROARCH.md) / kernel time / 1024 SIMDs (Little's law)",
                           "source": srcb + " (committed counter passes, not this run)"}
    return out


def reference_protocol_peak_mb(wl, dev):
    """Peak memory of one forward + backward the way the reference measures `max_mem_bw_kernel` (tests/utils.py:33-57,
    tests/renderer_speed_benchmark.py:158-180): inputs exist, NO gradient buffers yet; peak of allocated memory over forward +
    loss + backward relative to that base -- so outputs, saved state AND the gradient buffers count."""
    wl.zero_grads()
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    wl.loss(wl.forward(replicated=False)).backward()
    torch.cuda.synchronize(dev)
    return (torch.cuda.max_memory_allocated(dev) - base) / 2**20


# ----------------------------------------------------------------------------------------------------------------
# CPU baseline (the oracle = 'port' of the reference's naive path; test infrastructure, never the product)
# ----------------------------------------------------------------------------------------------------------------


def _time_cpu(one, budget_s, max_reps=50):
    one()
    t0 = time.perf_counter()
    reps = 0
    while reps < 3 or (time.perf_counter() - t0 < budget_s and reps < max_reps):
        one()
        reps += 1
    return (time.perf_counter() - t0) / reps, reps


def cpu_baseline(wl):
    import copy

    from oracle import lightplane_oracle as O
    from tests.synth import random_decoder, random_grids, random_rays

    torch.set_num_threads(min(16, os.cpu_count() or 1))  # more threads only thrash on problems this small
    cores = torch.get_num_threads()
    res = {"unit": "Mrays/s", "cores": cores, "kind": "port",
           "kind_note": "the reference itself (/root/reference, pure PyTorch) does not exist on the GPU box and cannot travel; the "
                        "oracle is its restatement, pinned to the fixtures the reference's own naive functions produced (tests/golden).  "
                        "Conservative: on cfg 1 the port is ~1.5x FASTER than the reference's lightplane_renderer_naive on the same "
                        "8 host cores (68.1 vs 44.6 ms fwd+bwd, measured by the round-4 review), so GPU / cpu_baseline understates "
                        "the ratio against the reference itself"}

    # BASELINE configs[0] ("cfg 1"): 1k random rays, 32^3 x 16 voxel grid, 64 samples, 2/2/2 x 32 decoder
    from tests.synth import baseline_cfg1
    d1 = baseline_cfg1()
    rays1, dec1, grids1 = d1["rays"], d1["decoder"], d1["grids"]

    def one_cfg1():
        rr = copy.copy(rays1)
        rr.encoding = rays1.encoding.clone().requires_grad_(True)
        d = copy.copy(dec1)
        d.mlp_params = dec1.mlp_params.clone().requires_grad_(True)
        gs = [g.clone().requires_grad_(True) for g in grids1]
        out = O.lightplane_renderer_naive(rr, gs, d, num_samples=64, gain=1.0)
        (out[0].sum() + out[1].sum() + out[2].sum()).backward()

    dt, reps = _time_cpu(one_cfg1, 6.0)
    res["cfg1"] = {"value": round(1000 / dt / 1e6, 6), "sample": f"BASELINE configs[0] exactly: 1000 random rays, 32^3x16 voxel, "
                   f"64 samples, 2/2/2x32 MLPs, fwd+bwd, {reps} reps"}

    n_sub = 1024
    if isinstance(wl, JointWorkload):
        res["value"], res["sample"] = res["cfg1"]["value"], res["cfg1"]["sample"]
        return res
    if isinstance(wl, RendererWorkload):
        idx = torch.arange(0, wl.n_rays, wl.n_rays // n_sub)[:n_sub]
        r = wl.rays_c[idx]

        def one():
            rr = copy.copy(r)
            rr.encoding = r.encoding.clone().requires_grad_(True)
            d = copy.copy(wl.dec_c)
            d.mlp_params = wl.dec_c.mlp_params.clone().requires_grad_(True)
            gs = [g.clone().requires_grad_(True) for g in wl.grids_c]
            out = O.lightplane_renderer_naive(rr, gs, d, num_samples=wl.S, gain=1.0)
            (out[0].sum() + out[1].sum() + out[2].sum()).backward()
    else:
        idx = torch.arange(0, wl.n_rays, wl.n_rays // n_sub)[:n_sub]
        r = wl.rays_c[idx]

        def one():
            rr = copy.copy(r)
            rr.encoding = r.encoding.clone().requires_grad_(True)
            out = O.lightplane_splatter_naive(rr, wl.sizes, num_samples=wl.S)
            out[0].sum().backward()

    dt, reps = _time_cpu(one, 10.0)
    res["value"] = round(n_sub / dt / 1e6, 6)
    res["sample"] = (f"{wl.name}-subsample: {n_sub} rays (every {wl.n_rays // n_sub}-th) of the benchmarked workload, fwd+bwd, "
                     f"{reps} reps, oracle/lightplane_oracle.py on CPU")
    return res


# ----------------------------------------------------------------------------------------------------------------


def measure_extra(name, dev, kernel, reps, **kw):
    """Short single-GPU measurement of another configuration (events only) for the `extras` block.  ``kw``: RendererWorkload
    switches (arithmetic=LP_ARITH_FP32: the reference's arithmetic; with_loss=True: the step protocol of rounds 1-4)."""
    wl = make_workload(name, 0, dev, None, kernel, **kw)
    for _ in range(2 if name in ("cfg4", "1080p_s128") else 10):
        wl.step()
    reps = max(reps, 5)
    torch.cuda.synchronize()
    fwd_ms, bwd_ms = event_times(wl, reps)
    peak_mb = reference_protocol_peak_mb(wl, dev)
    roof = wl.roofline(fwd_ms, bwd_ms)
    observed = soft(observed_kernels, wl, 2)
    if "error" in observed:
        observed = {}
    roof["binding"] = soft(binding_ceiling, name, wl, fwd_ms, bwd_ms, observed)
    relabel(roof)
    if roof["frac"] > 1.0 or roof["frac_fwd_plus_bwd"] > 1.0:
        roof["note"] = ("nominal line: SURVEY 8(d)'s algorithmic bytes are served by the L2 / Infinity Cache and merged in registers "
                        "before they reach the fabric, so a fraction above 1 is not a hardware limit exceeded -- see `binding`")
    out = {"workload": wl.desc, "rays": wl.n_rays, "fwd_ms": round(fwd_ms, 4), "bwd_ms": round(bwd_ms, 4),
           "Mrays_per_s_fwd_bwd": round(wl.n_rays / (fwd_ms + bwd_ms) / 1e3, 4), "reps": reps,
           "peak_bwd_mem_mb": round(peak_mb, 2), "roofline": roof}
    if isinstance(wl, RendererWorkload):
        out["mlp_fp32_frac_of_peak"] = round(wl.mlp_flops_fwdbwd() / ((fwd_ms + bwd_ms) * 1e-3) / FP32_PEAK, 5)
    if kw.get("arithmetic"):
        out["arithmetic"] = ("LP_ARITH_FP32 (LpRendererArgs.arithmetic, per call): " + _lib.build_info()["tuned_bwd"]["arith_fp32"] +
                             " -- the reference's arithmetic (triton_src/shared/const.py:9 ALLOW_TF32 = False); same forward kernel")
    if kw.get("with_loss"):  # wall time of whole steps: the loss kernels sit between the forward and the backward events
        for _ in range(3):
            wl.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = max(reps, 20)
        for _ in range(n):
            wl.step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / n * 1e3
        out.update(step_protocol="loss(out).backward() (rounds 1-4, reference tests/renderer_speed_benchmark.py:172-174)",
                   ms_per_step=round(ms, 4), Mrays_per_s_fwd_bwd=round(wl.n_rays / ms / 1e3, 4))
    del wl
    torch.cuda.empty_cache()
    return out


def measure_train_step(dev, kernel, reps=50):
    """The reference example's TRAINING ITERATION (its examples/fit_single_scene.py with examples/config/synthetic_overfit.json:
    --n_rays 4096 RANDOM rays per iteration, triplane 128^2 x 32 ch, S = 128, scaffold, mask_out_of_bounds_samples, decoder
    2/2/2 x 64): forward + MSE loss + backward issued back to back, events over ``reps`` iterations (scripts/bench_train_step.py is
    the standalone form with more sizes / both march orders; profiles/r06_train_step.txt)."""
    from tests.synth import grid_sizes_for, random_decoder, random_grids
    C, G, S, H = 32, 128, 128, 64
    gen = torch.Generator().manual_seed(0)
    dec0 = random_decoder(gen, 2, 2, 2, C, H, 3, std=0.15)
    params = dec0.mlp_params.to(dev).requires_grad_(True)
    dec = lp.DecoderParams(params, dec0.n_hidden_trunk, dec0.n_hidden_opacity, dec0.n_hidden_color, 3)
    grids = [g.to(dev).requires_grad_(True) for g in random_grids(gen, grid_sizes_for((1, G, G, G, C), True))]
    scaffold = (torch.rand(1, G, G, G, generator=gen) < 0.35).float().to(dev)
    out = {"workload": "reference examples/fit_single_scene.py + config/synthetic_overfit.json: n RANDOM rays per iteration, triplane "
                       "128^2 x 32 ch, S = 128, scaffold, decoder 2/2/2 x 64 (layer-looped family); forward + MSE loss + backward",
           "reps": reps, "rows": []}
    for n in (1024, 4096, 16384):
        o = torch.randn(n, 3, generator=gen) * 0.1 + torch.tensor([0.0, 0.0, 2.7])
        d = torch.nn.functional.normalize(torch.rand(n, 3, generator=gen) * 2 - 1 - o, dim=-1)
        rays = lp.Rays(directions=d.to(dev), origins=o.to(dev), grid_idx=torch.zeros(n, dtype=torch.int32, device=dev),
                       near=torch.full((n,), 1.0, device=dev), far=torch.full((n,), 4.4, device=dev),
                       encoding=torch.randn(n, H, generator=gen).to(dev).requires_grad_(True))
        target = torch.rand(n, 3, generator=gen).to(dev)

        def step():
            params.grad = rays.encoding.grad = None
            for g in grids:
                g.grad = None
            feat = lp.lightplane_renderer(rays, grids, dec, num_samples=S, gain=1.0, scaffold=scaffold, mask_out_of_bounds_samples=True,
                                          kernel=kernel)[2]
            ((feat - target) ** 2).mean().backward()

        for _ in range(5):
            step()
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            step()
        e1.record()
        torch.cuda.synchronize(dev)
        ms = e0.elapsed_time(e1) / reps
        out["rows"].append({"rays": n, "ms_per_iteration": round(ms, 4), "Mrays_per_s_fwd_bwd": round(n / ms / 1e3, 4)})
    out["Mrays_per_s_fwd_bwd"] = out["rows"][1]["Mrays_per_s_fwd_bwd"]  # the example's default: 4 096 rays
    torch.cuda.empty_cache()
    return out


def measure_cfg5(dev, kernel, reps=2):
    """BASELINE configs[4] at its per-GPU size on ONE GPU (13 views of 512 x 512 x 32 ch -> 256^3 x 32 ch voxel grid, 135 x 1920
    camera rows rendered from it at 256 samples, end-to-end backward through the render, the normalisation and the splat):
    event times, the kernels behind them (torch.profiler device times) and the peak memory of one step."""
    wl = JointWorkload(0, 1, dev, None, kernel)
    wl.step()
    torch.cuda.synchronize()
    fwd_ms, bwd_ms = event_times(wl, reps)
    peak_mb = reference_protocol_peak_mb(wl, dev)
    obs = observed_kernels(wl, 1)
    roof = wl.roofline(fwd_ms, bwd_ms)
    roof["binding"] = soft(cfg5_binding)
    roof["grid_tile_staging"] = GRID_TILE_STAGING
    out = {"workload": wl.desc, "rays": wl.n_rays, "splat_rays": wl.splat_rays.n_rays, "render_rays": wl.cam.n_rays,
           "fwd_ms": round(fwd_ms, 3), "bwd_ms": round(bwd_ms, 3), "Mrays_per_s_fwd_bwd": round(wl.n_rays / (fwd_ms + bwd_ms) / 1e3, 4),
           "reps": reps, "peak_bwd_mem_mb": round(peak_mb, 1), "roofline": roof,
           "kernels": {k: {"launches_per_step": v["launches_per_step"], "mean_ms": round(v["mean_ms"], 3)} for k, v in obs.items()},
           "timing": "HIP events around forward / backward (torch ops -- grid zero-fill, normalise, loss -- included); `kernels`: "
                     "torch.profiler device time of the lp:: kernels of one step"}
    del wl
    torch.cuda.empty_cache()
    return out


def kernel_times(wl, reps):
    """Median device time of the lp::renderer_fwd* / lp::renderer_bwd* kernels per step, from torch.profiler's device
    timestamps: for batches whose kernels are as short as the host side of a call, events around Python calls would
    measure the host."""
    from torch.profiler import ProfilerActivity, profile
    for _ in range(3):
        wl.step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            wl.step()
        torch.cuda.synchronize()
    per_kernel = {}  # kernel name -> device times of its launches (us)
    for e in prof.events():
        if e.device_type != torch.autograd.DeviceType.CUDA or not ("lp::renderer_fwd" in e.name or "lp::renderer_bwd" in e.name):
            continue
        per_kernel.setdefault(e.name.split("(")[0].replace("void ", ""), []).append(e.device_time_total)
    # median per kernel (a launch that shared the GPU with an allocator sync or a clock ramp does not move it), times the
    # launches per step
    med = {k: sorted(v)[len(v) // 2] * (len(v) / reps) for k, v in per_kernel.items()}
    kernel_times.last = {k: {"launches": len(v), "median_ms": round(sorted(v)[len(v) // 2] / 1e3, 4),
                             "max_ms": round(max(v) / 1e3, 4)} for k, v in per_kernel.items()}
    fwd = sum(t for k, t in med.items() if "renderer_fwd" in k)
    bwd = sum(t for k, t in med.items() if "renderer_bwd" in k)
    return fwd / 1e3, bwd / 1e3


def measure_small_batch(dev, kernel, reps):
    """A NeRF-style training batch (4 096 rays x 128 samples, cfg 2's grid and decoder): kernel times with the
    segment-parallel forward / backward (default; forward = segment march + combine pass) and with one sweep per ray."""
    wl = RendererWorkload("small", 0, dev, None, kernel)
    n_seg = lp.backward_segments(wl.rays, None, wl.dec, num_samples=wl.S, grid_sizes=wl.sizes)
    saved = lp.config.segment_backward, lp.config.segment_forward
    try:
        lp.config.segment_backward = lp.config.segment_forward = True
        f1, b1 = kernel_times(wl, reps)
        kernels = kernel_times.last
        lp.config.segment_backward = lp.config.segment_forward = False
        f0, b0 = kernel_times(wl, reps)
    finally:
        lp.config.segment_backward, lp.config.segment_forward = saved
    return {"workload": wl.desc, "rays": wl.n_rays, "backward_segments": n_seg, "fwd_ms": round(f1, 4), "bwd_ms": round(b1, 4),
            "bwd_ms_one_sweep_per_ray": round(b0, 4), "fwd_ms_one_sweep_per_ray": round(f0, 4), "reps": reps, "kernels": kernels,
            "timing": "torch.profiler device time of the lp:: kernels"}


def measure_sharded(name, rank, world, dev, pg, kernel, steps):
    """N > 1: one of the 1080p-per-rank configurations through the same ray-sharded step (grid / decoder gradients
    all-reduced over RCCL inside the step), timed like the headline: barrier + synchronize on both sides, max over ranks.
    Every rank runs this."""
    wl = make_workload(name, rank, dev, pg, kernel)
    wl.step()
    torch.distributed.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        wl.step()
    torch.distributed.barrier()
    torch.cuda.synchronize(dev)
    t = torch.tensor([time.perf_counter() - t0], device=dev, dtype=torch.float64)
    torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
    ms = float(t.item()) / steps * 1e3
    out = {"workload": wl.desc, "rays_per_gpu": wl.n_rays, "n_gpus": world, "steps": steps, "ms_per_step": round(ms, 3),
           "Mrays_per_s_fwd_bwd": round(wl.n_rays * world / ms / 1e3, 4)}
    del wl
    torch.cuda.empty_cache()
    return out


def relabel(roof):
    """Say what binds IN the record: when a `binding` block exists (instruction issue for the Renderer backward, atomic segments for
    the Splatter forward walk) `bound` names it and `binding_frac` carries its fraction; SURVEY 8(d)'s line (algorithmic bytes /
    time / 8 TB/s = achieved / peak / frac, the contract's fields) stays beside it as the NOMINAL hbm line -- cache-resident
    configurations exceed 1 there because run-merging and the L2 never move those bytes."""
    b = roof.get("binding")
    roof["nominal_hbm_frac"] = roof.get("frac")
    roof["bound_nominal"] = "hbm"
    if isinstance(b, dict) and b.get("kind") in ("issue", "atomic segments"):
        roof["bound"] = b["kind"]
        roof["binding_frac"] = b.get("frac_issue", b.get("frac_segments"))
    return roof


GRID_TILE_STAGING = {
    "built": False,
    "decision": "waived on evidence at the configuration where it could matter",
    "why": ("north_star names LDS staging of grid tiles.  Decided with counters on cfg 5's render leg, the one launch whose grid does NOT fit "
            "any cache (voxel 256^3 x 32 ch = 2.15 GB: 8x the Infinity Cache, 500x the L2; 135 x 1920 rays, 256 samples): L2 -> fabric fetch "
            "traffic of the forward is 0.17 GB per launch against 67.9 GB of algorithmic gather bytes (0.0025x), of the backward 0.23 GB "
            "(+ 0.60 GB of merged atomic segments) against 135.9 GB (0.006x); the backward's fetch phase is 4.2 k of 33.8 k cycles per "
            "wave-sample (12.5 %).  The round-5 review's criterion -- build it if fetch traffic > 1.5x algorithmic or the fetch phase > 25 % "
            "of the sample -- is missed by three orders of magnitude / a factor two: image-coherent rays re-read the rows their neighbours "
            "(lanes, and the previous sample) just pulled into the 32 KB L1 / 4 MB L2, which is exactly the reuse a staged tile would "
            "capture; a 128-ray workgroup's footprint (131 KB on an edge-on plane) would not fit the LDS left beside the weight images "
            "anyway.  cfg 2: FETCH_SIZE ~12 MB per backward launch against 12.9 GB.  Incoherent rays get their locality from the "
            "transposed march instead (consecutive samples of one ray per wavefront).  MLP weights ARE LDS staged (bf16x3 limb images)."),
    "evidence": ["profiles/r06_pmc_summary.json (cfg5: / cfg5_render: entries)", "profiles/r06_cfg5_render_phase_cycles.txt",
                 "profiles/r06_kernel_stats_cfg5.csv"],
}


def cfg5_binding(observed=None):
    """What binds the four kernels of cfg 5 (committed counter passes of `bench.py --workload cfg5`, profiles/rNN_pmc_summary.json):
    per kernel the L2 -> fabric traffic against the algorithmic bytes of SURVEY 8(d), the atomic-segment rate of the splat walk and
    the issue fraction of the render backward.  None when no counters are committed."""
    ns, nr, S, C = 13 * 512 * 512, 135 * 1920, 256, 32
    alg = {"splat_fwd_walk": ns * S * (8 * C * 4 + 8 * 4), "splat_bwd_walk": ns * S * 8 * C * 4,
           "renderer_fwd": nr * S * 8 * C * 4, "renderer_bwd": nr * S * 8 * C * 4 * 2}
    d0 = os.path.join(REPO, "profiles")
    files = [f for f in glob.glob(os.path.join(d0, "r*_pmc_summary.json")) if _PMC_FILE.search(os.path.basename(f))]
    files.sort(key=lambda f: int(_PMC_FILE.search(os.path.basename(f)).group(1)), reverse=True)
    for f in files:
        d = json.load(open(f))
        ent = {k.split(": ", 1)[1]: v for k, v in d.items() if k.startswith("cfg5: ") and "FETCH_SIZE" in v}
        if not ent:
            continue
        out = {"source": os.path.relpath(f, REPO) + " (committed counter passes, not this run)", "kernels": {}}
        for kn, v in ent.items():
            key = next((a for a in alg if a in kn), None)
            if key is None:
                continue
            ms = (v.get("trace_duration_ns") or v.get("pmc_duration_ns") or 0.0) / 1e6
            e = {"ms": round(ms, 3), "fetch_gb": round(v["FETCH_SIZE"] * 1024 / 1e9, 3), "write_gb": round(v.get("WRITE_SIZE", 0.0) * 1024 / 1e9, 3),
                 "algorithmic_gb": round(alg[key] / 1e9, 1),
                 "fabric_traffic_over_algorithmic": round((v["FETCH_SIZE"] + v.get("WRITE_SIZE", 0.0)) * 1024 / alg[key], 4)}
            if key == "splat_fwd_walk" and ms:
                segs = v["WRITE_SIZE"] * 1024 / 64.0
                e.update(kind="atomic segments", segments_per_launch=round(segs), frac_segments=round(segs / (ms * 1e-3) / ATOMIC_SEGMENTS_PER_S, 4))
            elif v.get("SQ_INSTS_VALU") and ms:
                clk = counter_clock_ghz(v) or CLOCK_GHZ
                e.update(kind="issue", frac_issue=round(v["SQ_INSTS_VALU"] * 4.0 / N_SIMD / (clk * 1e6) / ms, 4))
            out["kernels"][kn] = e
        out["kind"] = "per kernel: splat forward walk = atomic segments; the others = instruction issue; fabric traffic << algorithmic bytes everywhere"
        return out
    return None


def soft(fn, *a, **kw):
    """Run one optional leg of the bench; an exception becomes {"error": ...} instead of ending the run."""
    try:
        return fn(*a, **kw)
    except Exception as e:
        import traceback
        try:
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
        except Exception:
            pass
        return {"error": repr(e), "where": traceback.format_exc(limit=4).strip().splitlines()[-3:]}


EXTRAS = (  # key in `extras`, leg
    # the headline workload in the reference's arithmetic (three-limb dX chains, fp32 dW products), selected per call
    ("renderer_cfg2_fp32_arithmetic", lambda dev, k: measure_extra("cfg2", dev, k, 20, arithmetic=_lib.LP_ARITH_FP32)),
    # ... and with the step protocol of rounds 1-4 (scalar loss + its backward inside the step), once, for comparison across rounds
    ("headline_with_loss_kernels", lambda dev, k: measure_extra("cfg2", dev, k, 20, with_loss=True)),
    ("splatter_cfg3", lambda dev, k: measure_extra("cfg3", dev, k, 10)),
    ("renderer_1080p_s128", lambda dev, k: measure_extra("1080p_s128", dev, k, 5)),
    ("renderer_cfg4_shard", lambda dev, k: measure_extra("cfg4", dev, k, 5)),
    ("renderer_small_batch", lambda dev, k: measure_small_batch(dev, k, 20)),
    ("joint_cfg5_one_gpu", lambda dev, k: measure_cfg5(dev, k)),
    ("renderer_h64_example_112", lambda dev, k: measure_extra("h64_example_112", dev, k, 5)),
    ("renderer_h64_222", lambda dev, k: measure_extra("h64_222", dev, k, 5)),
    # the reference example's training iteration: 1 024 / 4 096 / 16 384 RANDOM rays through the example's decoder (latency-bound)
    ("renderer_train_step_example_h64", lambda dev, k: measure_train_step(dev, k)),
    # 65 536 RANDOM rays (the reference benchmark's 256^2 row as a steady-state workload): the backward's transposed march
    # (samples per wavefront), and the rays-per-wavefront kernel of rounds 1-5 on the same input for the A/B
    ("renderer_refbench256_random_rays", lambda dev, k: measure_extra("refbench256", dev, k, 10, march_order="samples")),
    ("renderer_refbench256_random_rays_march_rays", lambda dev, k: measure_extra("refbench256", dev, k, 5, march_order="rays")),
    # the reference's own benchmark axes (its protocol: wall time incl. host side, fresh inputs per rerun)
    ("refbench_renderer", lambda dev, k: refbench_renderer(dev, [256, 1024], k)),
    ("refbench_splatter", lambda dev, k: refbench_splatter(dev, [1, 16])),
)


def run_extras(dev, kernel, legs=EXTRAS):
    """The other configurations, one fail-soft leg each (N = 1, default workload)."""
    return {key: soft(leg, dev, kernel) for key, leg in legs}


DUMP_BYTES = 60 << 20  # all arrays of one --dump-outputs together (below 64 MB with the .npy headers)


def dump_outputs(arrays, out_dir, budget=DUMP_BYTES):
    """Write every array as out_dir/<name>.npy, float32 (float64 stays float64).  Smallest first, each array is written whole if
    it fits its share of what is left of the budget (the rest split evenly over the arrays still to come); a larger one is written
    as a fixed sample of its flattened elements: `share` indices drawn with seed 0, sorted -- the same for every run with the same
    arguments, so two builds are compared element for element.  Returns {name: (shape, elements written)}."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    items = sorted(((k, v.detach()) for k, v in arrays.items()), key=lambda kv: kv[1].numel())
    written = {}
    for i, (name, t) in enumerate(items):
        t = t if t.dtype == torch.float64 else t.float()
        share = budget // (len(items) - i) // t.element_size()
        if t.numel() > share:
            idx = torch.randint(0, t.numel(), (share,), generator=torch.Generator().manual_seed(0)).sort().values
            t = t.reshape(-1)[idx.to(t.device)]
        np.save(os.path.join(out_dir, name + ".npy"), t.cpu().numpy())
        budget -= t.numel() * t.element_size()
        written[name] = (list(arrays[name].shape), t.numel())
    return written


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default: >= 0.5 s of work: 200 for cfg2 / cfg3, "
                                                            "10 for the 1080p workloads)")
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--workload", default="cfg2", choices=["cfg2", "cfg4", "1080p_s128", "cfg3", "small", "cfg5", "refbench", "refbench_splatter", "h64_example_112", "h64_222", "refbench256", "cfg5_render"])
    ap.add_argument("--refbench-max", type=float, default=None, help="refbench: largest image size (default 2048) / refbench_splatter: "
                                                                      "largest num_view (default 256)")
    ap.add_argument("--kernel", type=int, default=_lib.LP_KERNEL_AUTO)
    ap.add_argument("--full", action="store_true", help="after the timed steps also measure fwd / bwd times, peak memory, roofline "
                                                        "and binding blocks, the other configurations (`extras`) and the CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-extras", action="store_true", help="--full without the runs of the other configurations")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the outputs and input gradients of the last timed step "
                                                                         "(rank 0) as DIR/<name>.npy, at most 64 MB in all")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL; gloo only to exercise the "
                                                       "multi-rank code path with several ranks on one GPU)")
    args = ap.parse_args()
    big = args.workload in ("cfg4", "1080p_s128", "h64_example_112", "h64_222", "refbench256", "cfg5_render")
    steps = args.steps if args.steps is not None else (2 if args.workload == "cfg5" else 10 if big else 200)
    warmup = args.warmup if args.warmup is not None else (1 if args.workload == "cfg5" else 2 if big else 10)
    if steps < 1 or warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.dump_outputs and args.workload in ("refbench", "refbench_splatter"):
        ap.error("--dump-outputs: the refbench tables draw fresh inputs per rerun and keep no outputs; use a timed-step workload")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` as a plain process: re-launch as N ranks (one per GPU) through torch.distributed.run
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        env.setdefault("OMP_NUM_THREADS", "8")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd, env=env))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    assert torch.cuda.is_available(), "bench.py needs a GPU (no CPU fallback)"
    dev = torch.device(f"cuda:{local_rank % torch.cuda.device_count()}")
    torch.cuda.set_device(dev)
    pg = None
    if world > 1:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(args.backend)
        pg = dist.group.WORLD
    if world != args.gpus and rank == 0:  # the launcher's world size is what runs; say so instead of dying
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}; running {world} rank(s)", file=sys.stderr, flush=True)

    global ARITHMETIC
    ARITHMETIC = arithmetic_string()
    lp.config.check_inputs = False  # the grid_idx range check is a host sync, not part of the op
    if args.workload in ("refbench", "refbench_splatter"):  # the reference's own benchmark tables (single GPU, its protocol; no timed-step loop)
        assert world == 1, "refbench is a single-GPU table"
        steps = args.steps if args.steps is not None else 5  # reruns per row (the reference's protocol: 2 warm-up + 5)
        warmup = args.warmup if args.warmup is not None else 2
        if args.workload == "refbench":
            tab = refbench_renderer(dev, [x for x in REFBENCH_SIZES if x <= (args.refbench_max or 2048) + 1e-6], args.kernel, steps, warmup)
            r = next((x for x in tab["rows"] if x["image_size"] == 256), tab["rows"][-1])
        else:
            tab = refbench_splatter(dev, [v for v in REFBENCH_VIEWS if v <= (args.refbench_max or 256)], steps, warmup)
            r = tab["rows"][0]
        print(json.dumps({"metric": f"Mrays/sec fwd+bwd ({args.workload}: the reference's speed benchmark, row image_size / num_view = "
                                    f"{r.get('image_size', r.get('num_view'))}); peak bwd mem (MB)",
                          "value": r["Mrays_per_s_fwd_bwd"], "unit": "Mrays/s", "n_gpus": 1, "steps": steps, "warmup": warmup,
                          "ms_per_step": round(r["t_fw_kernel_ms"] + r["t_bw_kernel_ms"], 4), "higher_is_better": True, "scaling": "weak",
                          "vs_baseline": None, "dtype": "f32", "arithmetic": ARITHMETIC, "data": "synthetic",
                          "config": {"workload": tab["benchmark"]}, "peak_bwd_mem_mb": r["max_mem_bw_kernel_mb"], "table": tab}), flush=True)
        return
    wl = make_workload(args.workload, rank, dev, pg, args.kernel)

    def sync():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize(dev)

    for _ in range(warmup):
        wl.step()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = wl.step()
    sync()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = float(t.item())
    ms_per_step = dt / steps * 1e3
    value = wl.n_rays * world / (ms_per_step * 1e-3) / 1e6
    if args.dump_outputs and rank == 0:
        dump_outputs(wl.results(out), args.dump_outputs)
    del out

    metric = ("Mrays/sec fwd+bwd, 64^3x16ch triplane @128 samples; peak bwd mem (MB)" if args.workload == "cfg2"
              else f"Mrays/sec fwd+bwd ({args.workload}); peak bwd mem (MB)")
    line = {"metric": metric, "value": round(value, 4), "unit": "Mrays/s", "n_gpus": world, "steps": steps, "warmup": warmup,
            "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "arithmetic": ARITHMETIC, "build": soft(build_record), "step_protocol": STEP_PROTOCOL, "data": "synthetic",
            "config": {"workload": wl.desc, "rays_per_gpu": wl.n_rays,
                       "parallelism": f"ray-shard dp{world}, grid replicated, "
                                      + ("un-normalised splat + weights all-reduced" if args.workload == "cfg3" else
                                         "splat grids summed (reduce-scatter + all-gather), render-grad all-reduce" if args.workload == "cfg5"
                                         else "grad all-reduce")}}
    if not args.full:  # the headline alone: nothing else runs on the GPU
        if rank == 0:
            print(json.dumps(line), flush=True)
        if world > 1:
            torch.distributed.destroy_process_group()
        return

    peak_mb = reference_protocol_peak_mb(wl, dev)  # outside the timed region; the reference's max_mem_bw protocol
    fwd_ms, bwd_ms = event_times(wl, max(5, min(steps, 20)))
    observed = soft(observed_kernels, wl, 3) if rank == 0 and not isinstance(wl, JointWorkload) else {}
    if "error" in observed:  # (the profiler pass only names the kernels; the timed numbers do not depend on it)
        observed = {}

    # N > 1, default workload: north_star's reporting batches (1920x1080 rays per GPU) through the same sharded step, so
    # that the driver's scaling runs carry them.  A watchdog bounds the leg: if it has not finished in time, rank 0
    # prints the headline line without it and every rank exits (a stuck collective cannot take the run with it).
    sharded = None
    watchdog_fired = []
    if world > 1 and args.workload == "cfg2" and not args.no_extras:  # (--full only)
        import threading
        done = threading.Event()
        line_ready = {}

        def bail():
            if done.is_set():
                return
            watchdog_fired.append(True)
            if rank == 0 and "res" in line_ready:
                r = dict(line_ready["res"])
                r["extras_error"] = "1080p legs did not finish within the watchdog limit"
                print(json.dumps(r), flush=True)
            os._exit(0)

        timer = threading.Timer(float(os.environ.get("LP_BENCH_EXTRAS_TIMEOUT", "240")), bail)
        timer.daemon = True
    else:
        timer = None

    def headline():
        roof = wl.roofline(fwd_ms, bwd_ms)
        dom = dominant_kernel(observed, "renderer_bwd" if isinstance(wl, RendererWorkload) else "splat_fwd_walk")
        traffic, src = pmc_traffic(args.workload, dom)
        roof["traffic"] = traffic
        roof["dominant_kernel"] = dom
        if dom and dom in observed:
            # one kernel, three clocks -- named, so that they cannot be mistaken for one another: torch.profiler's device timeline of
            # this run (instrumented: runs ~5-10 % long), HIP events around the whole backward of this run (`bwd_ms`, what `achieved`
            # uses), and rocprofv3's kernel trace of the committed profile pass
            roof["dominant_kernel_ms_torch_profiler"] = round(observed[dom]["mean_ms"], 4)
            pv, _, _ = pmc_entry(args.workload, dom)
            if pv and pv.get("trace_duration_ns"):
                roof["dominant_kernel_ms_rocprof_committed"] = round(pv["trace_duration_ns"] / 1e6, 4)
        roof["binding"] = soft(binding_ceiling, args.workload, wl, fwd_ms, bwd_ms, observed)
        relabel(roof)
        roof["traffic_source"] = (f"{src}: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command, NOT measured in "
                                  f"this run; L2 -> fabric requests, i.e. one 64 B write request per atomic segment") if src else None
        if isinstance(wl, RendererWorkload) and args.workload in ("cfg2", "1080p_s128"):
            roof["note"] = "effective bandwidth: the 786 KB grid is L2 resident, compulsory HBM bytes are ~0.5 KB/ray"
        if isinstance(wl, RendererWorkload):
            roof["grid_tile_staging"] = GRID_TILE_STAGING
        res = dict(line)
        res.update({
            "peak_bwd_mem_mb": round(peak_mb, 2),
            "peak_bwd_mem_protocol": "reference max_mem_bw_kernel (tests/utils.py:33-57): inputs resident, no gradient buffers yet; "
                                     "peak over forward + loss + backward (outputs, saved state and gradient buffers count)",
            "fwd_ms": round(fwd_ms, 4), "bwd_ms": round(bwd_ms, 4),
            "roofline": roof,
        })
        if isinstance(wl, RendererWorkload):
            res["mlp_fp32_frac_of_peak"] = round(wl.mlp_flops_fwdbwd() / ((fwd_ms + bwd_ms) * 1e-3) / FP32_PEAK, 5)
        return res

    def minimal_line(err):
        return {"metric": metric,
                "value": round(value, 4), "unit": "Mrays/s", "n_gpus": world, "steps": steps, "warmup": warmup,
                "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                "dtype": "f32", "arithmetic": ARITHMETIC, "data": "synthetic",
                "config": {"workload": getattr(wl, "desc", args.workload), "rays_per_gpu": wl.n_rays},
                "peak_bwd_mem_mb": round(peak_mb, 2), "fwd_ms": round(fwd_ms, 4), "bwd_ms": round(bwd_ms, 4),
                "roofline": soft(wl.roofline, fwd_ms, bwd_ms), "error": err}

    def headline_safe():
        try:
            return headline()
        except Exception as e:  # a helper of the annotated line failed: the measured numbers still go out
            return minimal_line("headline annotations failed: " + repr(e))

    if timer is not None:
        if rank == 0:
            line_ready["res"] = headline_safe()
        timer.start()
        sharded = {}
        for key, name, st in (("renderer_1080p_s128", "1080p_s128", 3), ("renderer_cfg4_shard", "cfg4", 2)):
            try:
                sharded[key] = measure_sharded(name, rank, world, dev, pg, args.kernel, st)
            except Exception as e:  # (a failing rank leaves the others in a collective: the watchdog ends the run)
                sharded[key] = {"error": repr(e)}
                break
        done.set()
        timer.cancel()

    if rank == 0:
        # The headline first; every further leg is optional and fails soft ({"error": ...}); the line is printed in a
        # `finally`, so nothing an extras / CPU leg does can take the driver's record with it.
        res = None
        try:
            res = headline_safe()
            if sharded is not None:
                res["extras"] = sharded
            if world == 1 and args.workload == "cfg2" and not args.no_extras:
                res["extras"] = run_extras(dev, args.kernel)
            if not args.no_cpu_baseline and world == 1:  # the CPU leg is reported at N = 1 only
                res["cpu_baseline"] = soft(cpu_baseline, wl)
        finally:
            if res is None:  # even headline_safe() failed: the contract fields alone
                res = minimal_line("headline assembly failed twice")
            print(json.dumps(res), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()

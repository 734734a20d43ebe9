"""Every tensor layout at the library's boundary, one small case per kernel path.

The other GPU tests hand the library tensors PyTorch has just allocated: dense, base 512-byte aligned.  Here the same VALUES arrive
* ``off4`` / ``off8``: as dense views one / two elements into a larger buffer (a parameter carved out of a flat parameter vector,
  ``encoding[1:]``): base 4 / 8 bytes past a 16-byte boundary.  The C ABI refuses such a pointer (tests/test_layout_host.py); the
  front-end copies the tensor to an aligned buffer first (``_lib.aligned``), so NO kernel here ever sees an under-aligned pointer;
* ``strided``: as non-contiguous views -- every other ray row, the leading columns of a wider encoding, every other element of a
  parameter buffer, grids stored channels-first and permuted, stride-0 upstream gradients (``(w * out).sum().backward()``).
In each variant EVERY float input is replaced at once and every differentiable input is a view of a base leaf.

Per case the baseline (fresh tensors) and the fp64 oracle are computed once.  Asserted: outputs and all gradients against the fp64
oracle at the project's 1e-4 of the largest entry; against the baseline -- Renderer / embedding forward bit-identical (no atomics),
splat outputs 2e-6, gradients 2e-5 (the run-to-run bars of test_grid_lists_are_zero_copy for "same values, other layout"); the base
leaf's gradient equals the baseline's on the view's elements and is exactly 0.0 on every element the view does not cover; the
grid-copy warning fires when, and only when, a grid is under-aligned.

Two graph-capture tests: a captured Renderer step on ``off4`` encoding / mlp_params, and a captured chain of the modular march on
``off4`` origins / directions, replay to the eager result on new contents of the buffers, so the realigning copy is part of the graph.

``JOB_IDS`` names every front-end of ``lightplane_amd.__all__`` that takes tensors, or the op has a boundary test of its own:
``calculate_scaffold`` / ``scaffold_opacity`` -- tests/test_gpu_scaffold.py::test_grid_layouts_at_the_boundary; ``marching_cubes`` /
``extract_mesh`` -- tests/test_gpu_mesh.py::test_layouts_are_refused; ``grid_resample`` / ``grid_up_sample`` --
tests/test_gpu_grid_resample.py::test_under_aligned_views_take_the_scalar_path_bit_for_bit; ``add_grid_tv_grad_`` shares the
``grid_tv`` job's front-end checks.  The jobs of the modular march and of the point ops live in tests/layout_jobs.py.

What a front-end does with an input that is not a fresh dense tensor -- the written contract (jobs in brackets):

    front-end                                  under-aligned (off4 / off8)                    not dense (strided)
    lightplane_renderer, LightplaneRenderer    copies; a grid: copies and warns               copies (a grid silently)
      [tuned .. scaffold, module_bg]
    lightplane_splatter, _mlp_splatter         copies; an input grid: copies and warns        copies
      [splat_*, mlp_splat*]
    ray embedding of the module                copies                                         copies
      [ray_embedding, module_bg]
    grid_tv_loss  [grid_tv]                    runs its scalar path, no copy                  refuses ("contiguous")
    ray_samples, composite_samples             copies                                         copies
      [ray_samples, composite]
    importance_samples  [importance]           copies                                         copies
    distortion_loss, interlevel_loss           copies                                         copies
      [distortion, interlevel]
    sample_grid_at_points                      copies; a grid: copies and warns               copies; a grid: refuses ("contiguous")
      [gather, gather_flat]
    splat_points  [splat_raw, splat_norm]      copies                                         copies
    lightplane_eval_mlp, _opacity_only         copies; a grid: REFUSES by the header's        copies; a grid: refuses ("contiguous")
      [points, points_opacity_scaffold]        name (``grid.grids[k].data``, ``grid.data``,
                                               ``color_grid...``), never copies
    LightplaneRenderer.eval_*_at_points        a grid: takes the Renderer path (copies, warns)  a grid: takes the Renderer path (copies)
    clip_rays_to_scaffold  [ray_clip]          copies; ``out=`` in place: REFUSES by name     refuses ("contiguous")
                                               (``rays.near_t``; ``near_out`` for a buffer
                                               of its own), never copies
    every upstream gradient                    copies                                         copies (stride 0 included)

The refusals have a test of their own (test_as_is_inputs_are_refused), as has the module's fallback; tests/test_layout_host.py holds
every ``_lib.aligned`` call of these front-ends to a mutation proof without a GPU.
"""
import contextlib
import dataclasses
import re
import warnings

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib
from lightplane_amd.modules import _RayEmbeddingFunction
from lightplane_amd.regularizers import grid_tv_loss
from oracle import lightplane_oracle as O
from tests.layout_jobs import NEW_JOBS, Job, PointsJob
from tests.layouts import VARIANTS, make_layout
from tests.synth import RENDERER_CASES, SPLATTER_CASES
from tests.test_gpu_grid_tv import ref_tv
from tests.test_gpu_parity import _assert_close, _dev, _rel_err

pytestmark = pytest.mark.gpu

F64 = torch.float64
RAY_FIELDS = ("directions", "origins", "near", "far")


@contextlib.contextmanager
def _config(**kw):
    old = {k: getattr(lp.config, k) for k in kw}
    for k, v in kw.items():
        setattr(lp.config, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(lp.config, k, v)


class RendererJob(Job):
    exact_forward = True

    def __init__(self, case, kernel=_lib.LP_KERNEL_AUTO, tag="", **config):
        self.name = f"renderer/{case}{tag}"
        self.kernel, self.config = kernel, config
        d = self.d = next(c for c in RENDERER_CASES if c.name == case).build()
        r = d["rays"]
        self.inputs = {f: (getattr(r, f), "rows", False, False) for f in RAY_FIELDS}
        self.inputs["encoding"] = (r.encoding, "columns", True, False)
        self.inputs["mlp_params"] = (d["decoder"].mlp_params, "rows", True, False)
        for i, g in enumerate(d["grids"]):
            self.inputs[f"grid{i}"] = (g, "grid", True, True)
        for i, g in enumerate(d["color_grids"] or []):
            self.inputs[f"color_grid{i}"] = (g, "grid", True, True)
        if d["scaffold"] is not None:
            self.inputs["scaffold"] = (d["scaffold"], "rows", False, False)

    def _args(self, t):
        d = self.d
        dev = t["encoding"].device
        rays = lp.Rays(directions=t["directions"], origins=t["origins"], grid_idx=d["rays"].grid_idx.to(dev), near=t["near"],
                       far=t["far"], encoding=t["encoding"])
        dec = d["decoder"]
        hdec = lp.DecoderParams(t["mlp_params"], dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
        grids = [t[f"grid{i}"] for i in range(len(d["grids"]))]
        cgrids = None if d["color_grids"] is None else [t[f"color_grid{i}"] for i in range(len(d["color_grids"]))]
        return rays, grids, hdec, dict(scaffold=t.get("scaffold"), color_grid=cgrids, **d["cfg"])

    def run(self, t, oracle=False):
        rays, grids, dec, kw = self._args(t)
        if oracle:
            return list(O.lightplane_renderer_naive(rays, grids, dec, **kw))
        return list(lp.lightplane_renderer(rays, grids, dec, kernel=self.kernel, **kw))


class ModuleJob(Job):
    """One step of the ``LightplaneRenderer`` module with the fused epilogue: ray-direction embedding kernel -> Renderer with the
    background colour and alpha composited in-kernel.  The module's parameters and buffer are replaced by the views."""
    exact_forward = True
    name = "module/LightplaneRenderer+bg_color"

    def __init__(self):
        gen = torch.Generator().manual_seed(77)
        torch.manual_seed(5)
        self.ctor = dict(num_samples=11, color_chn=3, grid_chn=16, mlp_hidden_chn=32, gain=2.0, opacity_init_bias=-1.0,
                         ray_embedding_num_harmonics=3)
        mod = lp.LightplaneRenderer(bg_color=0.0, **self.ctor)
        case = next(c for c in RENDERER_CASES if c.name == "triplane_basic")
        d = dataclasses.replace(case, n_rays=130).build()
        self.grid_idx = d["rays"].grid_idx
        r = d["rays"]
        self.inputs = {f: (getattr(r, f), "rows", False, False) for f in RAY_FIELDS}
        self.inputs["mlp_params"] = (mod.mlp_params.detach().clone() * 3.0, "rows", True, False)
        lin = mod.harmonic_ray_embedding_linear
        self.inputs["weight"] = (lin.weight.detach().clone(), "rows", True, False)
        self.inputs["bias"] = (0.1 * torch.randn(lin.bias.shape, generator=gen), "rows", True, False)
        self.inputs["bg_color"] = (torch.rand(3, generator=gen), "rows", False, False)
        for i, g in enumerate(d["grids"]):
            self.inputs[f"grid{i}"] = (0.7 * g, "grid", True, True)
        self.n_grids = len(d["grids"])

    def run(self, t, oracle=False):
        dev = t["weight"].device
        grids = [t[f"grid{i}"] for i in range(self.n_grids)]
        if oracle:
            # (the fp64 reference of the embedding is the package's own PyTorch op chain, calc_harmonic_embedding -> linear, and the
            # decoder layout comes from the module: not independent of the package, but independent of the HIP embedding kernel and
            # of the Renderer kernels, which are what runs on the other side)
            d = torch.nn.functional.normalize(t["directions"], dim=-1)
            enc = torch.nn.functional.linear(lp.calc_harmonic_embedding(d, 3), t["weight"], t["bias"])
            rays = lp.Rays(directions=t["directions"], origins=t["origins"], grid_idx=self.grid_idx, near=t["near"], far=t["far"], encoding=enc)
            mod = lp.LightplaneRenderer(bg_color=0.0, **self.ctor)
            dec = mod.get_decoder_params()
            dec = lp.DecoderParams(t["mlp_params"], dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
            length, nlt, feat = O.lightplane_renderer_naive(rays, grids, dec, num_samples=11, gain=2.0)
            T = torch.exp(-nlt)
            return [length, 1 - T, feat + T[..., None] * t["bg_color"]]
        mod = lp.LightplaneRenderer(bg_color=0.0, **self.ctor).to(dev)
        lin = mod.harmonic_ray_embedding_linear
        del mod.mlp_params, lin.weight, lin.bias  # (plain tensor attributes in the parameters' place: the views)
        mod.mlp_params, lin.weight, lin.bias = t["mlp_params"], t["weight"], t["bias"]
        rays = lp.Rays(directions=t["directions"], origins=t["origins"], grid_idx=self.grid_idx.to(dev), near=t["near"], far=t["far"])
        with _config(fused_module_ops=True):
            return list(mod(rays, grids, bg_color=t["bg_color"]))


class SplatterJob(Job):
    def __init__(self, case, kernel=_lib.LP_KERNEL_AUTO):
        c = next(c for c in SPLATTER_CASES if c.name == case)
        self.name = ("mlp_splatter/" if c.use_mlp else "splatter/") + case
        self.kernel = kernel
        d = self.d = c.build()
        r = d["rays"]
        self.inputs = {f: (getattr(r, f), "rows", False, False) for f in RAY_FIELDS}
        self.inputs["encoding"] = (r.encoding, "columns", True, False)
        if c.use_mlp:
            self.inputs["mlp_params"] = (d["mlp"].mlp_params, "rows", True, False)
            for i, g in enumerate(d["in_grids"]):
                self.inputs[f"in_grid{i}"] = (g, "grid", True, True)

    def run(self, t, oracle=False):
        d = self.d
        dev = t["encoding"].device
        rays = lp.Rays(directions=t["directions"], origins=t["origins"], grid_idx=d["rays"].grid_idx.to(dev), near=t["near"],
                       far=t["far"], encoding=t["encoding"])
        if d["mlp"] is None:
            fn = O.lightplane_splatter_naive if oracle else lp.lightplane_splatter
            return list(fn(rays, d["out_sizes"], **d["cfg"]))
        mlp = lp.SplatterParams(t["mlp_params"], d["mlp"].n_hidden)
        grids = [t[f"in_grid{i}"] for i in range(len(d["in_grids"]))]
        if oracle:
            return list(O.lightplane_mlp_splatter_naive(rays, d["out_sizes"], mlp, grids, **d["cfg"]))
        return list(lp.lightplane_mlp_splatter(rays, d["out_sizes"], mlp, grids, kernel=self.kernel, **d["cfg"]))


class EmbeddingJob(Job):
    exact_forward = True

    def __init__(self, n_h, e, n):
        self.name = f"ray_embedding/({n_h}, {e}, {n})"
        self.n_h = n_h
        gen = torch.Generator().manual_seed(n_h * 100 + e)
        self.inputs = {
            "directions": (torch.randn(n, 3, generator=gen) * torch.rand(n, 1, generator=gen) * 3, "rows", False, False),
            "weight": (torch.randn(e, 3 + 6 * n_h, generator=gen) * 0.3, "rows", True, False),
            "bias": (torch.randn(e, generator=gen) * 0.3, "rows", True, False),
        }

    def run(self, t, oracle=False):
        if oracle:  # (the package's own PyTorch op chain in fp64, as in ModuleJob: independent of the HIP kernel under test)
            d = torch.nn.functional.normalize(t["directions"], dim=-1)
            return [torch.nn.functional.linear(lp.calc_harmonic_embedding(d, self.n_h), t["weight"], t["bias"])]
        return [_RayEmbeddingFunction.apply(t["directions"], t["weight"], t["bias"], self.n_h)]


class GridTVJob(Job):
    """The total-variation regulariser keeps its own contract: an under-aligned grid runs its scalar path (4-byte accesses through a
    4-byte aligned pointer: nothing under-aligned for its type), a non-contiguous one is refused by the front-end."""
    name = "grid_tv/triplane+voxel"
    strided_raises = "contiguous"

    def __init__(self):
        gen = torch.Generator().manual_seed(3)
        self.w = [0.5, 2.0, 1.25, 0.7]
        shapes = [(2, 1, 7, 5), (2, 9, 1, 5), (2, 9, 7, 1), (2, 9, 7, 5)]
        self.inputs = {f"grid{i}": (torch.randn(*s, 16, generator=gen), "grid", True, False) for i, s in enumerate(shapes)}

    def run(self, t, oracle=False):
        grids = [t[f"grid{i}"] for i in range(len(self.w))]
        if oracle:
            return [ref_tv(grids, 1, self.w)]
        return [grid_tv_loss(grids, p=1, grid_weights=self.w)]


JOBS = [
    lambda: RendererJob("triplane_basic"),                                                   # tuned Renderer
    lambda: RendererJob("triplane_h64_c32"),                                                 # ... hidden 64 (two-block looped kernels)
    lambda: RendererJob("voxel_deep"),                                                       # layer-looped family
    lambda: RendererJob("colorgrid_c32_mixed"),                                              # separate colour grid
    lambda: RendererJob("triplane_basic", _lib.LP_KERNEL_GENERIC, "[generic]"),              # shape-generic kernels
    lambda: RendererJob("voxel_deep342_h64_c32", tag="[deep forward]", deep_forward_mfma=True),  # streamed deep forward, generic backward
    lambda: RendererJob("voxel_scaffold"),                                                   # a scaffold
    lambda: SplatterJob("triplane_basic"),
    lambda: SplatterJob("voxel_c64"),
    lambda: SplatterJob("mlp2_voxel"),
    lambda: SplatterJob("mlp3_voxel_h64_f32"),                                               # MLP-Splatter, looped family
    lambda: EmbeddingJob(3, 32, 300),
    lambda: ModuleJob(),
    lambda: GridTVJob(),
] + [make for _, make in NEW_JOBS]                                                           # the modular march and the point ops
JOB_IDS = ["tuned", "tuned_h64", "looped_deep", "colour_grid", "generic", "deep_forward", "scaffold", "splat_triplane", "splat_c64",
           "mlp_splat2", "mlp_splat3_h64", "ray_embedding", "module_bg", "grid_tv"] + [name for name, _ in NEW_JOBS]
_JOBS, _REF = {}, {}


def _job(i):
    if i not in _JOBS:
        _JOBS[i] = JOBS[i]()
    return _JOBS[i]


def _scalars(n):
    return [0.75 - 0.5 * k for k in range(n)]  # the scalar w of (w * out).sum(), one per output


def _upstream(job, outs, mode, seed=11):
    """One CPU tensor per output: N(0, 1) ("random") or the scalar w of ``(w * out).sum()`` in every entry ("const"), times the job's
    ``up_mask`` (the points the op's case file zeroes)."""
    gen = torch.Generator().manual_seed(seed)
    ups = []
    for k, (o, w) in enumerate(zip(outs, _scalars(len(outs)))):
        u = torch.randn(tuple(o.shape), generator=gen) if mode == "random" else torch.full(tuple(o.shape), w)
        m = job.up_mask(k)
        ups.append(u if m is None else u * m)
    return ups


def _masked(job, n_outs):
    return any(job.up_mask(k) is not None for k in range(n_outs))


def _same(a, b):
    """bit-identical (``torch.equal``, or the same bits where a NaN is part of the values)"""
    a, b = a.detach().cpu(), b.detach().cpu()
    if torch.equal(a, b):
        return True
    return a.dtype == b.dtype == torch.float32 and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _grads(outs, ups, leaves, retain):
    pairs = [(o, u) for o, u in zip(outs, ups) if o.requires_grad]  # (an output without a gradient stays out of the backward)
    got = torch.autograd.grad([o for o, _ in pairs], leaves, [u for _, u in pairs], retain_graph=retain, allow_unused=True)
    return [torch.zeros_like(l) if g is None else g for g, l in zip(got, leaves)]


def _reference(i, dev):
    """Computed once per job, shared by its variants and left unchanged: the baseline on fresh tensors and the fp64 oracle, outputs and
    the gradients for both upstream flavours -- "random" (off4 / off8) and "const" (``torch.full_like(out, w)``: what the strided
    variant's ``(w * out).sum().backward()`` means)."""
    if i in _REF:
        return _REF[i]
    job = _job(i)
    names = [n for n, (_, _, diff, _) in job.inputs.items() if diff]
    ref = {}
    for which in ("baseline", "oracle"):
        if which == "baseline":
            t = {n: v.to(dev).clone().requires_grad_(diff) for n, (v, _, diff, _) in job.inputs.items()}
            with _config(**job.config), warnings.catch_warnings():
                warnings.simplefilter("ignore", UserWarning)
                outs = job.run(t)
        else:
            t = {n: (v.to(F64) if v.dtype.is_floating_point else v).clone().requires_grad_(diff) for n, (v, _, diff, _) in job.inputs.items()}
            old = torch.get_num_threads()
            torch.set_num_threads(min(16, old))
            try:
                outs = job.run(t, oracle=True)
            finally:
                torch.set_num_threads(old)
        ref[which] = dict(outs=[o.detach().cpu() for o in outs])
        if names:
            leaves = [t[n] for n in names]
            for mode, retain in (("random", True), ("const", False)):
                g = _grads(outs, [u.to(o) for u, o in zip(_upstream(job, outs, mode), outs)], leaves, retain)
                ref[which][mode] = dict(zip(names, (x.cpu() for x in g)))
    _REF[i] = ref
    return ref


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("i", range(len(JOBS)), ids=JOB_IDS)
def test_layout_variant(i, variant, monkeypatch):
    dev = _dev()
    job = _job(i)
    ref = _reference(i, dev)
    mode = "const" if variant == "strided" else "random"
    lay = {n: make_layout(v, variant, kind, seed=k) for k, (n, (v, kind, _, _)) in enumerate(job.inputs.items())}
    base, t = {}, {}
    for n, (v, _, diff, _) in job.inputs.items():
        base[n], t[n] = lay[n].on(dev, diff)
        assert _same(t[n].to(v.dtype), v), n
        if lay[n].identity:  # (an input the front-end takes in no other layout: the docstring of tests/layouts.py::make_layout)
            assert t[n].is_contiguous() and t[n].data_ptr() % 16 == 0, n
        elif variant == "strided":
            assert not t[n].is_contiguous(), f"{n}: the strided view is dense"
        else:
            assert t[n].is_contiguous() and t[n].data_ptr() % 16 == (4 if variant == "off4" else 8), n
    if variant == "strided" and job.strided_raises:
        with pytest.raises(AssertionError, match=job.strided_raises):
            job.run(t)
        return
    # the copy of a grid is announced: when a grid is under-aligned, and only then
    monkeypatch.setattr(_lib, "_grid_clone_warned", False)
    expect_warning = variant != "strided" and any(is_grid for (_, _, _, is_grid) in job.inputs.values())
    with _config(**job.config), warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        if expect_warning:
            with pytest.warns(UserWarning, match="not 16-byte aligned"):
                outs = job.run(t)
        else:
            outs = job.run(t)
    assert expect_warning or not [w for w in rec if "16-byte aligned" in str(w.message)], "grid-copy warning without an under-aligned grid"
    # backward: off4 / off8 upstream gradients at an element offset themselves; strided: the stride-0 expansion autograd makes (where
    # the job zeroes the upstream gradient at some points, the same constants times its mask as every other row of a larger tensor)
    diff_outs = [k for k, o in enumerate(outs) if o.requires_grad]
    assert bool(diff_outs) == any(diff for (_, _, diff, _) in job.inputs.values()), "differentiable inputs and no differentiable output"
    if not diff_outs:
        pass
    elif variant == "strided" and not _masked(job, len(outs)):
        sum((w * o).sum() for k, (w, o) in enumerate(zip(_scalars(len(outs)), outs)) if k in diff_outs).backward()
    else:
        ups = []
        for k, u in enumerate(_upstream(job, outs, mode)):
            _, uv = make_layout(u, variant, seed=100 + k).on(dev)
            if variant == "strided":
                assert not uv.is_contiguous()
            else:
                assert uv.data_ptr() % 16 in (4, 8) and uv.is_contiguous()
            ups.append(uv)
        torch.autograd.backward([outs[k] for k in diff_outs], [ups[k] for k in diff_outs])
    torch.cuda.synchronize()
    bl, orc = ref["baseline"], ref["oracle"]
    job.meets_oracle(f"{job.name}[{variant}]", outs, orc["outs"])
    for k, o in enumerate(outs):
        nm = f"{job.name}[{variant}] out{k}"
        if job.exact_forward:
            assert _same(o, bl["outs"][k]), f"{nm}: not bit-identical to the baseline"
        else:
            print(f"{nm}: vs baseline {_rel_err(o, bl['outs'][k].numpy()):.3e}")
            _assert_close(nm + "/baseline", o, bl["outs"][k].numpy(), job.out_tol)
    for n, (v, _, diff, _) in job.inputs.items():
        if not diff:
            continue
        nm = f"{job.name}[{variant}] grad {n}"
        g = base[n].grad
        assert g is not None and g.shape == base[n].shape, f"{nm}: no gradient on the base leaf"
        on_view = lay[n].view(g)
        print(f"{nm}: vs oracle {_rel_err(on_view, orc[mode][n].numpy()):.3e}, vs baseline {_rel_err(on_view, bl[mode][n].numpy()):.3e}")
        _assert_close(nm + "/oracle", on_view, orc[mode][n].numpy())
        _assert_close(nm + "/baseline", on_view, bl[mode][n].numpy(), 2e-5)
        off_view = g.cpu()[~lay[n].covered()]
        assert off_view.numel() > 0 or lay[n].identity or (variant == "strided" and job.inputs[n][1] == "grid"), (
            f"{nm}: the view covers its whole base")
        assert off_view.numel() == 0 or float(off_view.abs().max()) == 0.0, (
            f"{nm}: gradient leaked to {int((off_view != 0).sum())} elements of the base tensor the view does not cover")


def test_baseline_meets_the_oracle():
    """The reference point of the variants is itself right: every job's baseline against its fp64 oracle (1e-4 of the largest entry)."""
    dev = _dev()
    for i in range(len(JOBS)):
        ref = _reference(i, dev)
        _job(i).meets_oracle(_job(i).name, ref["baseline"]["outs"], ref["oracle"]["outs"])
        for mode in ("random", "const"):
            for n in ref["baseline"].get(mode, ()):
                _assert_close(f"{_job(i).name} grad {n} ({mode})", ref["baseline"][mode][n], ref["oracle"][mode][n].numpy())


def test_graph_capture_realigns_inside_the_graph():
    """A Renderer step on an ``off4`` encoding and ``off4`` mlp_params captures into a HIP graph (the pattern of
    test_gpu_parity.py::test_hip_graph_capture_of_forward_backward: one stream, no parallel branches, ``check_inputs`` off) and replays
    to the eager result AFTER the buffers' contents changed: the realigning copy is part of the graph, not hoisted out of it at
    capture time.

    The leaves carry no autograd history from outside the step (the views are cut inside it): a view of a leaf made on the default
    stream and kept alive keeps the leaf's AccumulateGrad node on that stream, the captured backward then hops to the default stream
    and the capture never joins it -- ending such a capture crashes the process.  PyTorch warns about that mismatch; here the warning
    is an error, raised by the warm-up before any capture begins."""
    dev = _dev()
    with _config(check_inputs=False), warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*AccumulateGrad node's stream")
        d = next(c for c in RENDERER_CASES if c.name == "triplane_basic").build()
        dec = d["decoder"]
        r = d["rays"].to(dev)
        enc_shape, par_shape = tuple(r.encoding.shape), tuple(dec.mlp_params.shape)
        n_enc, n_par = r.encoding.numel(), dec.mlp_params.numel()
        enc_base = make_layout(r.encoding.cpu(), "off4").base_cpu.to(dev).requires_grad_(True)
        par_base = make_layout(dec.mlp_params, "off4").base_cpu.to(dev).requires_grad_(True)
        flat = lp.flatten_grid([g.to(dev) for g in d["grids"]])[0].requires_grad_(True)
        leaves = (flat, par_base, enc_base)

        def step():
            enc, par = enc_base[1: 1 + n_enc].view(enc_shape), par_base[1: 1 + n_par].view(par_shape)
            assert enc.data_ptr() % 16 == 4 and par.data_ptr() % 16 == 4 and enc.is_contiguous() and par.is_contiguous()
            rays = lp.Rays(directions=r.directions, origins=r.origins, grid_idx=r.grid_idx, near=r.near, far=r.far, encoding=enc)
            hdec = lp.DecoderParams(par, dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
            o = lp.lightplane_renderer(rays, flat, hdec, grid_sizes=d["sizes"], **d["cfg"])
            (o[0].sum() + o[1].sum() + o[2].sum()).backward()
            return [t.detach() for t in o]

        def clear():
            for t in leaves:
                t.grad = None

        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                clear()
                step()
        torch.cuda.current_stream().wait_stream(s)
        clear()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            outs = step()
        # new contents in the captured buffers: what a copy hoisted out of the graph would miss
        with torch.no_grad():
            enc_base.mul_(0.5).add_(0.25)
            par_base.mul_(1.5)
        for t in leaves:
            t.grad.zero_()
        g.replay()
        torch.cuda.synchronize()
        got_out = [o.clone() for o in outs]
        got = [t.grad.clone() for t in leaves]
        clear()
        want_out = step()
        torch.cuda.synchronize()
        for nm, a, b in zip(("ray_length", "neg_log_t", "feature"), got_out, want_out):
            assert torch.equal(a, b), f"graph replay {nm} differs from the eager step on the same contents"
        for nm, a, t in zip(("grid", "params", "encoding"), got, leaves):
            _assert_close(f"graph replay grad_{nm}", a, t.grad.cpu().numpy(), 1e-5)
        assert float(par_base.grad[0]) == 0.0 and float(enc_base.grad[0]) == 0.0


# ---- inputs the front-ends hand over as they are: refused by name, never copied ------------------------------------------------------


def _job_named(name):
    if name == "points_twogrid":  # (a colour grid-list; not one of JOBS: its layout variants are the "points" job's)
        if name not in _JOBS:
            _JOBS[name] = PointsJob("voxel_c32_twogrid_022x32")
        return _JOBS[name]
    return _job(JOB_IDS.index(name))


_IN_PLACE, _OUT_BUFFER = "out[0] is rays.near", "out[0] is a buffer of its own"
#: (job, input, variant, the field the library's message begins with)
REFUSALS = (
    [("points", f"grid{k}", v, f"grid.grids[{k}].data") for k in range(3) for v in VARIANTS]
    + [("points_opacity_scaffold", "grid", v, "grid.data") for v in VARIANTS]
    + [("points_twogrid", "color_grid0", v, "color_grid.grids[0].data") for v in VARIANTS]
    # (the gather copies an under-aligned grid -- the variants of its job -- and refuses one that is not dense)
    + [("gather", "grid1", "strided", None), ("gather_flat", "grid", "strided", None)]
    + [("ray_clip", f, "strided", None) for f in ("directions", "origins", "near", "far", "gidx", "scaffold")]
    # (in place the result pointer IS the ray's: the library checks the ray's fields first and names that one)
    + [("ray_clip", _IN_PLACE, v, "rays.near_t") for v in ("off4", "off8")]
    + [("ray_clip", _OUT_BUFFER, v, "near_out") for v in ("off4", "off8")]
)


@pytest.mark.parametrize("jid, inp, variant, field", REFUSALS, ids=[f"{j}-{i}-{v}".replace(" ", "_") for j, i, v, _ in REFUSALS])
def test_as_is_inputs_are_refused(jid, inp, variant, field):
    """An input a front-end hands to the library as it is -- the grids of ``lightplane_eval_mlp`` / ``_opacity_only``, the results of
    ``clip_rays_to_scaffold(out=...)`` -- is refused when it is under-aligned, by the library and by the name the header gives the
    field, and when it is not dense, by the front-end ("contiguous"): never copied behind the caller's back.  Nothing was launched or
    left half-written: the next valid call on the same stream gives the result of the call before, bit for bit."""
    dev = _dev()
    job = _job_named(jid)

    def fresh():
        return {n: v.to(dev).clone() for n, (v, _, _, _) in job.inputs.items()}

    def refused(call):
        match = "contiguous" if variant == "strided" else re.escape(field) + " .*16-byte aligned"
        with pytest.raises(AssertionError, match=match):
            call()

    with torch.no_grad(), warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*16-byte aligned")  # (nothing is copied: no copy is announced either)
        want = job.run(fresh())
        t = fresh()
        if inp in (_IN_PLACE, _OUT_BUFFER):
            n = t["near"].shape[0]
            far_o, hit_o = torch.full((n,), 7.0, device=dev), torch.full((n,), 7, dtype=torch.uint8, device=dev)
            values = job.inputs["near"][0] if inp == _IN_PLACE else torch.full((n,), 7.0)
            _, near_o = make_layout(values, variant).on(dev)
            if inp == _IN_PLACE:
                t["near"] = near_o
            refused(lambda: job.run(t, out=(near_o, far_o, hit_o)))
            torch.cuda.synchronize()
            assert _same(near_o, values) and float((far_o - 7.0).abs().max()) == 0.0 and int((hit_o != 7).sum()) == 0, "a refused call wrote"
        else:
            v, kind = job.inputs[inp][:2]
            _, t[inp] = make_layout(v, variant, "grid" if kind in ("as_is", "offset_only") else kind).on(dev)
            assert _same(t[inp].to(v.dtype), v)
            assert not t[inp].is_contiguous() if variant == "strided" else t[inp].data_ptr() % 16 in (4, 8)
            refused(lambda: job.run(t))
        got = job.run(fresh())
        torch.cuda.synchronize()
        assert len(got) == len(want) and all(_same(a, b) for a, b in zip(got, want)), "the call after a refusal differs from the one before"


def test_ray_clip_in_place_on_aligned_rays_is_the_out_of_place_result():
    """``out=(rays.near, rays.far, hit)`` with aligned ray fields: accepted, written in place, and bit for bit what the call without
    ``out`` returns."""
    dev = _dev()
    job = _job_named("ray_clip")
    with torch.no_grad():
        want = job.run({n: v.to(dev).clone() for n, (v, _, _, _) in job.inputs.items()})
        t = {n: v.to(dev).clone() for n, (v, _, _, _) in job.inputs.items()}
        assert t["near"].data_ptr() % 16 == 0 and t["far"].data_ptr() % 16 == 0
        hit_o = torch.empty(t["near"].shape[0], dtype=torch.uint8, device=dev)
        near, far, hit = job.run(t, out=(t["near"], t["far"], hit_o))
        torch.cuda.synchronize()
    assert near is t["near"] and far is t["far"]
    assert _same(near, want[0]) and _same(far, want[1]) and _same(hit, want[2]) and _same(hit_o.bool(), want[2])
    assert not _same(near, job.inputs["near"][0]), "nothing was clipped: the in-place call shows nothing"


def test_module_falls_back_for_layouts_the_fused_path_refuses(monkeypatch):
    """``LightplaneRenderer.eval_opacity_at_points`` / ``eval_decoder_at_points`` with a grid-list the fused functions refuse -- ``off4``
    views, channels-first permuted tensors -- take the Renderer path, whose front-end copies: the fused functions are not called, and
    the results meet the fp64 oracle at the bar the fused path meets on fresh tensors."""
    from lightplane_amd import modules
    from tests.test_gpu_points import _module_inputs
    dev = _dev()
    mod, grids, _, pts, gidx, enc = _module_inputs(dev)
    calls = []

    def spy(name):
        fn = getattr(modules, name)

        def wrapped(*a, **kw):
            calls.append(name)
            return fn(*a, **kw)
        monkeypatch.setattr(modules, name, wrapped)

    spy("_fused_eval_mlp")
    spy("_fused_eval_mlp_opacity_only")
    dec = mod.get_decoder_params()
    dec64 = lp.DecoderParams(dec.mlp_params.detach().cpu().double(), dec.n_hidden_trunk.cpu(), dec.n_hidden_opacity.cpu(), dec.n_hidden_color.cpu(), 3)
    o_op, o_col = O.eval_decoder(pts.double(), [g.double() for g in grids], gidx, dec64, enc.double(), 2.0)
    dpts, didx, denc = pts.to(dev), gidx.to(dev), enc.to(dev)
    assert lp.config.fused_module_ops
    layouts = {"fresh": [g.to(dev) for g in grids], "off4": [make_layout(g, "off4", seed=k).on(dev)[1] for k, g in enumerate(grids)],
               "channels_first": [make_layout(g, "strided", "grid", seed=k).on(dev)[1] for k, g in enumerate(grids)]}
    assert all(g.data_ptr() % 16 == 4 for g in layouts["off4"]) and not any(g.is_contiguous() for g in layouts["channels_first"])
    for which, dg in layouts.items():
        del calls[:]
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)  # (the Renderer's front-end announces its copy of an under-aligned grid)
            op = mod.eval_opacity_at_points(dpts, didx, dg)
            op2, col = mod.eval_decoder_at_points(dpts, didx, denc, dg)
        if which == "fresh":
            assert calls == ["_fused_eval_mlp_opacity_only", "_fused_eval_mlp"], f"the fused functions were not what ran: {calls}"
        else:
            assert calls == [], f"{which}: the fused path was taken: {calls}"
        for nm, got, want in (("opacity", op, o_op), ("opacity (joint)", op2, o_op), ("colour", col, o_col[..., :3])):
            print(f"{which} {nm}: vs oracle {_rel_err(got, want.numpy()):.3e}")
            _assert_close(f"{which} {nm}", got, want.numpy())


def test_graph_capture_of_a_modular_chain_realigns_inside_the_graph():
    """test_graph_capture_realigns_inside_the_graph for the modular march: ``ray_samples -> sample_grid_at_points -> softplus of the
    feature sum as opacity -> composite_samples(return_weights=True) -> distortion_loss`` on ``off4`` origins and directions, backward
    of the loss plus the rendered feature, captured with the same precautions (views cut inside the step, one stream, three warm-ups on a
    side stream, the AccumulateGrad-stream warning an error).  The replay on NEW contents of the off4 buffers is the eager step on those
    contents: outputs bit for bit, gradients to the 1e-5 of that test (the grid gradient is a splat: atomics), and element 0 of each
    base leaf -- which the view does not cover -- keeps a gradient of exactly 0."""
    from tests.synth import grid_sizes_for, random_rays
    dev = _dev()
    n_rays, n_samples = 63, 9
    with _config(check_inputs=False), warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*AccumulateGrad node's stream")
        gen = torch.Generator().manual_seed(23)
        r = random_rays(gen, n_rays, 2, None)
        grids = [(0.5 * torch.randn(s, generator=gen)).to(dev).requires_grad_(True) for s in grid_sizes_for((2, 6, 5, 7, 16), True)]
        org_base = make_layout(r.origins, "off4").base_cpu.to(dev).requires_grad_(True)
        dir_base = make_layout(r.directions, "off4", seed=1).base_cpu.to(dev).requires_grad_(True)
        near, far, gidx = r.near.to(dev), r.far.to(dev), r.grid_idx.to(dev)
        leaves = (org_base, dir_base, *grids)

        def step():
            org, drc = org_base[1: 1 + 3 * n_rays].view(n_rays, 3), dir_base[1: 1 + 3 * n_rays].view(n_rays, 3)
            assert org.data_ptr() % 16 == 4 and drc.data_ptr() % 16 == 4 and org.is_contiguous() and drc.is_contiguous()
            smp = lp.ray_samples(lp.Rays(directions=drc, origins=org, grid_idx=gidx, near=near, far=far), n_samples)
            feat = lp.sample_grid_at_points(smp.points, grids, gidx)
            opacity = torch.nn.functional.softplus(feat.sum(-1))
            length, nlt, feature, w = lp.composite_samples(opacity, feat, smp.depths, smp.deltas, return_weights=True)
            loss = lp.distortion_loss(w, smp.depths, smp.deltas)
            (loss.sum() + feature.sum()).backward()
            return [t.detach() for t in (length, nlt, feature, w, loss)]

        def clear():
            for t in leaves:
                t.grad = None

        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                clear()
                step()
        torch.cuda.current_stream().wait_stream(s)
        clear()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            outs = step()
        # new contents in the captured buffers: what a copy hoisted out of the graph would miss
        with torch.no_grad():
            org_base.mul_(0.5).add_(0.125)
            dir_base.mul_(1.25)
        for t in leaves:
            t.grad.zero_()
        g.replay()
        torch.cuda.synchronize()
        got_out = [o.clone() for o in outs]
        got = [t.grad.clone() for t in leaves]
        clear()
        want_out = step()
        torch.cuda.synchronize()
        for nm, a, b in zip(("ray_length", "neg_log_t", "feature", "weights", "distortion"), got_out, want_out):
            assert torch.equal(a, b), f"graph replay {nm} differs from the eager step on the same contents"
        for nm, a, t in zip(("origins", "directions", "grid0", "grid1", "grid2"), got, leaves):
            assert float(t.grad.abs().max()) > 0.0
            _assert_close(f"graph replay grad_{nm}", a, t.grad.cpu().numpy(), 1e-5)
        for nm, a in zip(("origins", "directions"), got):
            assert float(a[0]) == 0.0 and float(a[1:].abs().max()) > 0.0, f"graph replay grad_{nm}: element 0 of the base leaf"
        assert float(org_base.grad[0]) == 0.0 and float(dir_base.grad[0]) == 0.0

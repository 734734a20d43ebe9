"""CPU tests of the memory-layout contract (no GPU, no kernel launch).

* The C ABI refuses every device pointer that is not 16-byte aligned (include/lightplane_hip.h, Conventions) -- every pointer field of
  the three argument blocks, found from the ctypes struct definitions, on every entry point, before anything touches the device
  (fake pointers, ``n_rays == 0``).
* ``_lib.aligned``: the Python front-end's answer -- an aligned tensor passes through, a dense view at an element offset into a larger
  buffer is copied; the copy of a grid warns once per process.
* Mutation proof: with ``lib()`` replaced by a recorder, every pointer the wrappers hand over for inputs at a 4-byte aligned base is
  16-byte aligned, and with ``_lib.aligned`` replaced by the identity every one of those call sites hands over the under-aligned
  pointer -- the helper alone stands between such an input and the kernels, and a dropped call is noticed.  Four drives: the Renderer
  and the Splatter, the MLP-Splatter and the ray embedding, the modular march (ray_samples, composite_samples, importance_samples, both
  ray losses) and the point ops (gather, splat, ``lightplane_eval_mlp``, the ray clip).  Three kinds of pointer: the wrappers' own
  buffers (``_OWN`` / ``_OWN_BY_ENTRY``: always aligned), the caller's inputs (aligned by the helper, the caller's own pointer without
  it) and ``AS_IS`` -- the few inputs a front-end hands over uncopied on purpose, the caller's pointer in both proofs.
"""
import contextlib
import ctypes
import re
import warnings

import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib, grids, params
from lightplane_amd.modules import _RayEmbeddingFunction
from tests.layouts import get_slot, offset_layout, pointer_fields, set_slot, snapshot
from tests.synth import RENDERER_CASES, SPLATTER_CASES

FAKE = 0x7F0000010000  # never dereferenced: n_rays == 0


def _fill_fake_pointers(a):
    """Every pointer slot of the block gets its own fake 16-byte aligned address."""
    for k, (_, owner, key) in enumerate(pointer_fields(a)):
        set_slot(owner, key, FAKE + 0x100 * k)
    return a


def _renderer_args():
    a = _lib.LpRendererArgs()
    a.rays.n_rays = 0
    a.rays.encoding_dim = 32
    a.grid = _lib.make_grid_list(None, [grids.GridDesc(1, 4, 4, 4, 0)], 16, 64)
    a.scaffold_shape = _lib.LpGrid(1, 4, 4, 4, 0, None)
    a.march = _lib.make_march(8, 0, False, False, 1e-5)
    dims = ([16, 32, 32], [32, 32, 1], [32, 32, 16])
    n = [params.mlp_numel(d) for d in dims]
    a.trunk, a.opacity, a.color = _lib.make_mlp(dims[0], 0), _lib.make_mlp(dims[1], n[0]), _lib.make_mlp(dims[2], n[0] + n[1])
    a.n_mlp_params = sum(n)
    a.color_chn = 3
    a.alpha_mode = 1  # (alpha / grad_alpha are given)
    return _fill_fake_pointers(a)


def _splatter_args(mlp: bool):
    a = _lib.LpSplatterArgs()
    a.rays.n_rays = 0
    a.rays.encoding_dim = 32
    a.march = _lib.make_march(8, 0, False, False, 1e-5)
    a.out = _lib.make_grid_list(None, [grids.GridDesc(1, 4, 4, 4, 0)], 32, 64)
    if mlp:
        a.input_grid = _lib.make_grid_list(None, [grids.GridDesc(1, 3, 4, 5, 0)], 32, 60)
        a.mlp = _lib.make_mlp([32, 32, 32], 0)
        a.n_mlp_params = params.mlp_numel([32, 32, 32])
    return _fill_fake_pointers(a)


def _embed_args():
    e = _lib.LpRayEmbedArgs()
    e.n_rays, e.n_harmonics, e.out_dim = 0, 3, 32
    return _fill_fake_pointers(e)


def _entry_points():
    """(id, argument block builder, call, path filter).  ``call(L, a)`` -> return code."""
    ref = ctypes.byref
    dump = FAKE + 0x8000  # (relu-dump twins: [n_rays = 0][S][W] words at a fake aligned address)
    return [
        ("lp_renderer_forward", _renderer_args, lambda L, a: L.lp_renderer_forward(ref(a), None), None),
        ("lp_renderer_backward", _renderer_args, lambda L, a: L.lp_renderer_backward(ref(a), None), None),
        ("lp_renderer_forward_ws", _renderer_args, lambda L, a: L.lp_renderer_forward_ws(ref(a), FAKE, 0, None), None),
        ("lp_renderer_backward_relu_dump", _renderer_args, lambda L, a: L.lp_renderer_backward_relu_dump(ref(a), dump, 0, None), None),
        ("lp_splatter_forward", lambda: _splatter_args(False), lambda L, a: L.lp_splatter_forward(ref(a), None), None),
        ("lp_splatter_backward", lambda: _splatter_args(False), lambda L, a: L.lp_splatter_backward(ref(a), None), None),
        ("lp_splatter_forward[mlp]", lambda: _splatter_args(True), lambda L, a: L.lp_splatter_forward(ref(a), None), None),
        ("lp_splatter_backward[mlp]", lambda: _splatter_args(True), lambda L, a: L.lp_splatter_backward(ref(a), None), None),
        ("lp_mlp_splatter_backward_relu_dump", lambda: _splatter_args(True),
         lambda L, a: L.lp_mlp_splatter_backward_relu_dump(ref(a), dump, 0, None), None),
        ("lp_ray_embedding_forward", _embed_args, lambda L, a: L.lp_ray_embedding_forward(ref(a), None), None),
        ("lp_ray_embedding_backward", _embed_args, lambda L, a: L.lp_ray_embedding_backward(ref(a), None), None),
        # the parity hook reads the rays only (check_rays): its ray pointers follow the rule as well
        ("lp_renderer_corner_rows", _renderer_args, None, "rays."),
    ]


ENTRY_POINTS = _entry_points()


def test_the_walk_finds_every_pointer_of_the_argument_blocks():
    """The field list comes from the struct definitions: as many slots as the header declares pointers (a slot the walk missed would be a
    slot the alignment test never shifts)."""
    got = {st.__name__: [p for p, _, _ in pointer_fields(st())] for st in (
        _lib.LpRays, _lib.LpGridList, _lib.LpRendererArgs, _lib.LpSplatterArgs, _lib.LpRayEmbedArgs, _lib.LpPointsArgs, _lib.LpPointGridArgs,
        _lib.LpRayClipArgs, _lib.LpRaySamplesArgs, _lib.LpCompositeArgs, _lib.LpImportanceArgs, _lib.LpDistortionArgs, _lib.LpInterlevelArgs)}
    assert got["LpRays"] == ["directions", "origins", "grid_idx", "near_t", "far_t", "encoding"]
    assert len(got["LpGridList"]) == 1 + _lib.LP_MAX_GRIDS
    # LpRendererArgs: rays 6, two grid-lists 2 x 9, scaffold + scaffold_shape.data, mlp_params, 3 outputs, ckpt, 3 upstream grads,
    # 4 flat gradient buffers, 2 x 8 list entries, bg_color, alpha, grad_alpha, seg_prefix
    assert len(got["LpRendererArgs"]) == 6 + 18 + 2 + 1 + 3 + 1 + 3 + 4 + 16 + 4
    assert len(got["LpSplatterArgs"]) == 6 + 18 + 2 + 1 + 5 + 8
    assert len(got["LpRayEmbedArgs"]) == 7
    assert "grid.grids[7].data" in got["LpRendererArgs"] and "grad_color_grid_list[7]" in got["LpRendererArgs"]
    # LpPointsArgs (lightplane_hip.h): two grid-lists 2 x 9, mlp_params, points + grid_idx + encoding, scaffold + scaffold_shape.data,
    # 2 outputs + 2 upstream grads, 2 flat grid gradients, 2 x 8 list entries, grad_mlp_params + grad_encoding + grad_points
    assert len(got["LpPointsArgs"]) == 18 + 1 + 3 + 2 + 4 + 2 + 16 + 3
    # LpPointGridArgs: grid-list 9, row_weight[8], points + grid_idx, vectors + out_features + grad_points
    assert len(got["LpPointGridArgs"]) == 9 + 8 + 2 + 3
    # LpRayClipArgs: rays 6, scaffold + scaffold_shape.data (near_out / far_out / hit_out are arguments of lp_rays_clip, not fields)
    assert len(got["LpRayClipArgs"]) == 6 + 2
    # lightplane_hip_samples.h -- LpRaySamplesArgs: rays 6, 3 results, 3 upstream grads, 4 gradients; LpCompositeArgs: 4 inputs,
    # 4 results, 4 upstream grads, 4 gradients
    assert len(got["LpRaySamplesArgs"]) == 6 + 3 + 3 + 4
    assert len(got["LpCompositeArgs"]) == 4 + 4 + 4 + 4
    # lightplane_hip_importance.h -- 5 inputs, 3 results, grad_points, 2 gradients
    assert len(got["LpImportanceArgs"]) == 5 + 3 + 1 + 2
    # lightplane_hip_losses.h -- LpDistortionArgs: 3 inputs, grad_loss + loss, 3 gradients; LpInterlevelArgs: 4 inputs, grad_loss +
    # loss, 1 gradient
    assert len(got["LpDistortionArgs"]) == 3 + 2 + 3
    assert len(got["LpInterlevelArgs"]) == 4 + 2 + 1
    assert "row_weight[7]" in got["LpPointGridArgs"] and "color_grid.grids[7].data" in got["LpPointsArgs"]
    assert "rays.near_t" in got["LpRayClipArgs"] and "rays.far_t" in got["LpRaySamplesArgs"]
    for paths in got.values():
        assert len(set(paths)) == len(paths)


@pytest.mark.parametrize("entry", [e for e in ENTRY_POINTS if e[2] is not None], ids=lambda e: e[0])
def test_zero_rays_over_aligned_pointers_is_ok(entry):
    """Aligned pointers everywhere and no rays: validated, nothing launched, LP_OK -- on every entry point."""
    name, build, call, _ = entry
    L = _lib.lib()
    rc = call(L, build())
    assert rc == 0, f"{name}: rc {rc}: {L.lp_last_error().decode()}"


def _corner_rows_call(L, a):
    return L.lp_renderer_corner_rows(ctypes.byref(a), FAKE + 0x9000, None)


@pytest.mark.parametrize("entry", ENTRY_POINTS, ids=lambda e: e[0])
def test_every_under_aligned_pointer_is_refused_by_name(entry):
    """One pointer field at a time, 4, 8 and 12 bytes off: LP_EINVAL, and the message begins with that field as the header spells it.
    No field is exempt: the list is every pointer slot of the struct definition."""
    name, build, call, only = entry
    call = call or _corner_rows_call
    L = _lib.lib()
    paths = [p for p, _, _ in pointer_fields(build())]
    if only is not None:
        paths = [p for p in paths if p.startswith(only)]
    assert paths
    for path in paths:
        for shift in (4, 8, 12):
            a = build()
            owner, key = next((o, k) for p, o, k in pointer_fields(a) if p == path)
            set_slot(owner, key, get_slot(owner, key) + shift)
            rc = call(L, a)
            msg = L.lp_last_error().decode()
            assert rc == -1, f"{name}: {path} + {shift} bytes: rc {rc} ({msg})"
            assert msg.startswith(path + " ") and "16-byte aligned" in msg, f"{name}: {path} + {shift} bytes: {msg!r}"


def test_splatter_normalize_refuses_under_aligned_buffers():
    L = _lib.lib()
    assert L.lp_splatter_normalize(FAKE, FAKE + 0x100, 0, 32, None) == 0
    for k, field in enumerate(("feature", "weight")):
        for shift in (4, 8, 12):
            p = [FAKE, FAKE + 0x100]
            p[k] += shift
            assert L.lp_splatter_normalize(p[0], p[1], 0, 32, None) == -1
            msg = L.lp_last_error().decode()
            assert msg.startswith(field + " ") and "16-byte aligned" in msg, msg


def test_null_pointers_and_row_offsets_are_not_pointers_to_align():
    """NULL stays legal wherever it was (the rule is about non-NULL pointers), and a grid at an odd row offset of a flat tensor with
    C % 4 != 0 channels -- a row address that is 4-byte aligned only -- is not refused: row offsets are not pointers."""
    L = _lib.lib()
    a = _lib.LpRendererArgs()
    a.rays.n_rays, a.rays.encoding_dim = 0, 32
    a.grid = _lib.make_grid_list(None, [grids.GridDesc(1, 1, 3, 3, 0), grids.GridDesc(1, 3, 1, 3, 9)], 3, 18)
    a.grid.data = FAKE
    a.march = _lib.make_march(8, 0, False, False, 1e-5)
    dims = ([3, 32, 32], [32, 32, 1], [32, 32, 16])
    n = [params.mlp_numel(d) for d in dims]
    a.trunk, a.opacity, a.color = _lib.make_mlp(dims[0], 0), _lib.make_mlp(dims[1], n[0]), _lib.make_mlp(dims[2], n[0] + n[1])
    a.n_mlp_params, a.color_chn, a.mlp_params = sum(n), 3, FAKE + 0x100
    assert L.lp_renderer_forward(ctypes.byref(a), None) == 0, L.lp_last_error()


# ---- the Python helper ----------------------------------------------------------------------------------------------------------


def test_aligned_returns_the_tensor_or_an_equal_aligned_copy(monkeypatch):
    buf = torch.arange(64, dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    assert _lib.aligned(buf) is buf and _lib.aligned(None) is None
    v4 = buf[4:]
    assert _lib.aligned(v4) is v4  # an offset of a multiple of four floats keeps the alignment: no copy
    for k in (1, 2, 3):
        v = buf[k: k + 40].view(8, 5)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4 * k
        c = _lib.aligned(v)
        assert c is not v and c.data_ptr() % 16 == 0 and c.is_contiguous() and torch.equal(c, v)
        assert c.data_ptr() != v.data_ptr()
    e = torch.empty(0)
    assert _lib.aligned(e) is e


def test_the_clone_of_a_grid_warns_once_per_process(monkeypatch):
    monkeypatch.setattr(_lib, "_grid_clone_warned", False)
    buf = torch.zeros(1 + 2 * 3 * 4 * 5 * 4)
    g = buf[1:].view(2, 3, 4, 5, 4)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        _lib.aligned(buf[1:9])                       # not a grid: silent
        _lib.aligned(buf[4:].view(-1)[:16], grid=True)  # an aligned grid: silent
        assert not rec
        a = _lib.aligned(g, grid=True)
        b = _lib.aligned(g, grid=True)
    assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
    assert len(rec) == 1 and "16-byte aligned" in str(rec[0].message) and issubclass(rec[0].category, UserWarning)


# ---- mutation proof: the helper alone aligns what the wrappers hand over ---------------------------------------------------------


class _Recorder:
    """Stands in for the loaded library: every entry point records its arguments (argument blocks as private copies) and returns 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            snap = []
            for x in args:
                obj = getattr(x, "_obj", None)
                snap.append(snapshot(obj) if isinstance(obj, ctypes.Structure) else x)
            self.calls.append((name, snap))
            return 0
        return fn

    def all_pointers(self):
        """[((entry point, field path), pointer)] over every non-NULL pointer of every recorded call."""
        out = []
        for name, args in self.calls:
            for x in args:
                if isinstance(x, ctypes.Structure):
                    for path, owner, key in pointer_fields(x):
                        p = get_slot(owner, key)
                        if p:
                            out.append(((name, path), p))
            if name == "lp_splatter_normalize":
                out += [((name, "feature"), args[0]), ((name, "weight"), args[1])]
            if name == "lp_rays_clip":  # (args, near_out, far_out, hit_out, stream)
                out += [((name, field), p) for field, p in zip(("near_out", "far_out", "hit_out"), args[1:4])]
        return out

    def pointers(self):
        """{(entry point, field path): pointer}: the first call that gave the field a non-NULL pointer."""
        out = {}
        for k, p in self.all_pointers():
            out.setdefault(k, p)
        return out


@pytest.fixture
def recorder(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(_lib, "current_stream", lambda dev: None)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(_lib, "_grid_clone_warned", False)
    return rec


def _off4(t, requires_grad=False):
    """The values of ``t`` as a dense CPU view whose base is 4 bytes past a 16-byte boundary."""
    base, v = offset_layout(t, 1).on("cpu", requires_grad)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _off4_rays(rays):
    return lp.Rays(directions=_off4(rays.directions), origins=_off4(rays.origins), grid_idx=_off4(rays.grid_idx.to(torch.int32)),
                   near=_off4(rays.near), far=_off4(rays.far), encoding=_off4(rays.encoding, True))


#: pointer fields whose buffers the wrappers allocate themselves (outputs, saved state, gradient buffers): always fresh allocations.
#: Every OTHER non-NULL pointer of a recorded call is a caller's tensor.
_OWN = re.compile(r"^(ray_length|neg_log_t|feature|neg_log_t_ckpt|alpha|seg_prefix|out\.data|out_feature|out_weight|weight|out"
                  r"|grad_(grid|color_grid|mlp_params|encoding|input_grid|weight|bias)|grad_(grid|color_grid|input_grid)_list\[\d\])$")
_GRID_FIELDS = r"grid\.data|grid\.grids\[\d\]\.data"
_OWN_BY_ENTRY = {"lp_ray_embedding_forward": ("out",), "lp_ray_embedding_backward": ("grad_weight", "grad_bias"),
                 "lp_splatter_normalize": ("feature", "weight"),
                 # the modular march (compositing.py, importance.py, ray_losses.py): results; gradients; of the saved tensors the
                 # importance backward's ``out_depths`` is a result of the forward (every other saved tensor is an input's aligned copy
                 # with the helper and the caller's tensor without it: an input)
                 "lp_ray_samples_forward": ("points", "depths", "deltas"),
                 "lp_ray_samples_backward": ("grad_origins", "grad_directions", "grad_near", "grad_far"),
                 "lp_composite_forward": ("ray_length", "neg_log_t", "feature", "weights"),
                 "lp_composite_backward": ("grad_opacity", "grad_features", "grad_depths", "grad_deltas"),
                 "lp_importance_samples_forward": ("out_points", "out_depths", "out_deltas"),
                 "lp_importance_samples_backward": ("out_depths", "grad_origins", "grad_directions"),
                 "lp_distortion_forward": ("loss",), "lp_distortion_backward": ("grad_weights", "grad_depths", "grad_deltas"),
                 "lp_interlevel_forward": ("loss",), "lp_interlevel_backward": ("grad_proposal_weights",),
                 # gather / splat at points (point_grid.py): the gather reads a caller's grid-list (the grids; a splat's upstream grids)
                 # and writes features, dividing by the splat's saved ``row_weight``; the splat and the normalisation write a grid-list
                 # of the wrapper's own (the result; the gather's grid gradient)
                 "lp_point_gather": re.compile(r"out_features|row_weight\[\d\]"),
                 "lp_point_splat": re.compile(_GRID_FIELDS + r"|row_weight\[\d\]"),
                 "lp_point_normalize": re.compile(_GRID_FIELDS + r"|row_weight\[\d\]"),
                 "lp_point_grad_points": ("grad_points",),
                 # the decoder at points (points.py)
                 "lp_points_forward": ("opacity_out", "color_out"),
                 "lp_points_backward": re.compile(r"grad_(grid|color_grid|mlp_params|encoding|points)|grad_(grid|color_grid)_list\[\d\]"),
                 # the ray clip (ray_clip.py): the three results, unless they are the caller's ``out=`` in place (AS_IS)
                 "lp_rays_clip": ("near_out", "far_out", "hit_out")}

#: (entry point, fields) whose pointer is the CALLER'S in both proofs, helper or not, and why.  The drives name the pointers they expect
#: there; a pointer at one of these fields that is not one of those is classified like any other.
AS_IS = {
    ("lp_points_forward", "lp_points_backward"): (
        re.compile(r"(color_)?(" + _GRID_FIELDS + ")"),
        "lightplane_eval_mlp hands grids over as they are (a grid of GBs is never copied behind the caller's back); the library refuses "
        "an under-aligned one by name (tests/test_points_host.py, tests/test_gpu_layouts.py::test_as_is_inputs_are_refused)"),
    ("lp_rays_clip",): (
        re.compile(r"near_out|far_out|rays\.near_t|rays\.far_t"),
        "out=(rays.near, rays.far, hit): the results have to land in the caller's own tensors, so neither side of the alias can be "
        "copied; the library refuses an under-aligned one by name"),
}


def _as_is_rule(entry, path):
    for entries, (fields, _) in AS_IS.items():
        if entry in entries and fields.fullmatch(path):
            return True
    return False


def _is_input(entry, path):
    if entry in _OWN_BY_ENTRY:
        own = _OWN_BY_ENTRY[entry]
        return not own.fullmatch(path) if isinstance(own, re.Pattern) else path not in own
    if entry.startswith("lp_splatter") and path == "weight":
        return False  # the splat weights the forward saved
    return not _OWN.match(path)


def _drive_every_wrapper():
    """Forward + backward of every wrapper that hands pointers to the library, EVERY tensor input -- upstream gradients included -- at a
    4-byte aligned base (CPU tensors: the library is the recorder).  Returns the (entry point, field) pairs that have to show up."""
    from lightplane_amd.renderer import _render, renderer_corner_rows
    sites = []
    fwd, bwd = "lp_renderer_forward", "lp_renderer_backward"
    ray_sites = ["rays." + f for f in ("directions", "origins", "grid_idx", "near_t", "far_t")]
    # Renderer, grid-list + scaffold + fused epilogue (background colour, alpha)
    d = next(c for c in RENDERER_CASES if c.name == "voxel_scaffold").build()
    rays = _off4_rays(d["rays"])
    dec = d["decoder"]
    hdec = lp.DecoderParams(_off4(dec.mlp_params, True), dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
    gs = [_off4(g, True) for g in d["grids"]]
    n = rays.n_rays
    out = _render(rays, gs, hdec, scaffold=_off4(d["scaffold"]), bg_color=_off4(torch.rand(3)), alpha_mode=1, **d["cfg"])
    torch.autograd.backward(list(out), [_off4(torch.randn(n)), _off4(torch.randn(n)), _off4(torch.randn(n, 3)), _off4(torch.randn(n))])
    sites += [(fwd, f) for f in ["grid.grids[0].data", "mlp_params", "rays.encoding", "scaffold", "bg_color"] + ray_sites]
    sites += [(bwd, f) for f in ("grad_ray_length", "grad_neg_log_t", "grad_feature", "grad_alpha")]
    # ... two-grid decoder: as lists of three planes each, then as flat tensors
    d = next(c for c in RENDERER_CASES if c.name == "colorgrid_c32_mixed").build()
    dec = d["decoder"]
    n = d["rays"].n_rays
    flat, sizes = lp.flatten_grid(d["grids"])
    cflat, csizes = lp.flatten_grid(d["color_grids"])
    for as_list in (True, False):
        hdec = lp.DecoderParams(_off4(dec.mlp_params, True), dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)
        if as_list:
            out = lp.lightplane_renderer(_off4_rays(d["rays"]), [_off4(g, True) for g in d["grids"]], hdec,
                                         color_grid=[_off4(g, True) for g in d["color_grids"]], **d["cfg"])
        else:
            out = lp.lightplane_renderer(_off4_rays(d["rays"]), _off4(flat, True), hdec, grid_sizes=sizes.tolist(),
                                         color_grid=_off4(cflat, True), color_grid_sizes=csizes.tolist(), **d["cfg"])
        torch.autograd.backward(list(out), [_off4(torch.randn(n)), _off4(torch.randn(n)), _off4(torch.randn(n, 3))])
    sites += [(e, f"{gl}.grids[{k}].data") for e in (fwd, bwd) for gl in ("grid", "color_grid") for k in range(3)]
    sites += [(e, f"{gl}.data") for e in (fwd, bwd) for gl in ("grid", "color_grid")]
    # the corner-row parity hook
    renderer_corner_rows(_off4_rays(d["rays"]), d["sizes"], 4)
    sites += [("lp_renderer_corner_rows", f) for f in ray_sites]
    # plain Splatter
    ds = next(c for c in SPLATTER_CASES if c.name == "triplane_basic").build()
    out = lp.lightplane_splatter(_off4_rays(ds["rays"]), ds["out_sizes"], return_list=False, **ds["cfg"])
    out.backward(_off4(torch.randn(out.shape)))
    sites += [("lp_splatter_forward", f) for f in ["rays.encoding"] + ray_sites] + [("lp_splatter_backward", "grad_out")]
    return sites


def _drive_mlp_splatter_and_embedding():
    """(The MLP-Splatter in its own record: its entry points are the plain Splatter's.)  Input grid-list of three planes, then flat."""
    sites = []
    sf, sb = "lp_splatter_forward", "lp_splatter_backward"
    dm = next(c for c in SPLATTER_CASES if c.name == "mlp2_triplane_c16").build()
    flat, sizes = lp.flatten_grid(dm["in_grids"])
    for as_list in (True, False):
        mlp = lp.SplatterParams(_off4(dm["mlp"].mlp_params, True), dm["mlp"].n_hidden)
        grid = [_off4(g, True) for g in dm["in_grids"]] if as_list else _off4(flat, True)
        out = lp.lightplane_mlp_splatter(_off4_rays(dm["rays"]), dm["out_sizes"], mlp, grid, return_list=False,
                                         input_grid_sizes=None if as_list else sizes.tolist(), **dm["cfg"])
        out.backward(_off4(torch.randn(out.shape)))
    sites += [(sf, "rays.encoding"), (sf, "mlp_params"), (sb, "grad_out"), (sf, "input_grid.data"), (sb, "input_grid.data")]
    sites += [(e, f"input_grid.grids[{k}].data") for e in (sf, sb) for k in range(3)]
    # ray-direction embedding of the module front-end
    lin = torch.nn.Linear(3 + 6 * 3, 32)
    w, b = _off4(lin.weight.detach(), True), _off4(lin.bias.detach(), True)
    out = _RayEmbeddingFunction.apply(_off4(torch.randn(30, 3)), w, b, 3)
    out.backward(_off4(torch.randn(30, 32)))
    ef, eb = "lp_ray_embedding_forward", "lp_ray_embedding_backward"
    sites += [(ef, "directions"), (ef, "weight"), (ef, "bias"), (eb, "grad_out"), (eb, "directions")]
    return sites


def _drive_the_modular_march():
    """ray_samples, composite_samples, importance_samples and both ray losses, forward and backward: every input and every upstream
    gradient at a 4-byte aligned base.  (Small shapes of the ops' own case files: nothing is launched.)"""
    from tests import compositing_cases as CC
    from tests import importance_cases as IC
    from tests import ray_loss_cases as LC
    from tests.synth import random_rays
    sites = []
    n, s_reg, s_inf, chn, n_new, n_prop = 7, 4, 1, 4, 3, 6
    s = s_reg + s_inf
    ray_sites = ["rays." + f for f in ("directions", "origins", "near_t", "far_t")]
    # ray_samples
    r = random_rays(torch.Generator().manual_seed(1), n, 2, None)
    rays = lp.Rays(directions=_off4(r.directions, True), origins=_off4(r.origins, True), grid_idx=r.grid_idx, near=_off4(r.near, True),
                   far=_off4(r.far, True))
    out = lp.ray_samples(rays, s_reg, s_inf)
    torch.autograd.backward(list(out), [_off4(torch.randn(n, s, 3)), _off4(torch.randn(n, s)), _off4(torch.randn(n, s))])
    sites += [(e, f) for e in ("lp_ray_samples_forward", "lp_ray_samples_backward") for f in ray_sites]
    sites += [("lp_ray_samples_backward", f) for f in ("grad_points", "grad_depths", "grad_deltas")]
    # composite_samples with features and weights
    c = CC.inputs(n, s, chn, "mixed")
    names = ("opacity", "features", "depths", "deltas")
    out = lp.composite_samples(*(_off4(c[k], True) for k in names), return_weights=True)
    torch.autograd.backward(list(out), [_off4(torch.randn(n)), _off4(torch.randn(n)), _off4(torch.randn(n, chn)), _off4(torch.randn(n, s))])
    sites += [(e, f) for e in ("lp_composite_forward", "lp_composite_backward") for f in names]
    sites += [("lp_composite_backward", f) for f in ("grad_ray_length", "grad_neg_log_t", "grad_feature", "grad_weights")]
    # importance_samples with jitter
    c = IC.inputs(n, s, n_new, "transparent")
    rays = lp.Rays(directions=_off4(c["directions"], True), origins=_off4(c["origins"], True), grid_idx=r.grid_idx, near=r.near, far=r.far)
    out = lp.importance_samples(rays, _off4(c["depths"]), _off4(c["weights"]), n_new, jitter=_off4(c["jitter"]))
    out.points.backward(_off4(torch.randn(n, s + n_new, 3)))
    sites += [("lp_importance_samples_forward", f) for f in ("origins", "directions", "depths", "weights", "jitter")]
    sites += [("lp_importance_samples_backward", f) for f in ("directions", "grad_points")]
    # distortion_loss
    c = LC.distortion_inputs(n, s, "mixed")
    names = ("weights", "depths", "deltas")
    lp.distortion_loss(*(_off4(c[k], True) for k in names)).backward(_off4(torch.randn(n)))
    sites += [(e, f) for e in ("lp_distortion_forward", "lp_distortion_backward") for f in names] + [("lp_distortion_backward", "grad_loss")]
    # interlevel_loss
    c = LC.interlevel_inputs(n, s, n_prop, "violating")
    names = ("weights", "depths", "proposal_weights", "proposal_depths")
    lp.interlevel_loss(*(_off4(c[k], k == "proposal_weights") for k in names)).backward(_off4(torch.randn(n)))
    sites += [(e, f) for e in ("lp_interlevel_forward", "lp_interlevel_backward") for f in names] + [("lp_interlevel_backward", "grad_loss")]
    return sites


def _drive_the_point_ops():
    """The gather in list and flat form, the raw and the normalised splat, ``lightplane_eval_mlp`` with a scaffold and a colour
    grid-list, its opacity-only twin on a flat grid, and the ray clip -- on its default path and in place.  Returns the sites and the
    AS_IS pointers: ``{(entry point, field): the caller's pointers expected there}``."""
    from tests import point_grid_cases as GC
    from tests import points_cases as PC
    from tests import ray_clip_cases as RC
    sites, as_is = [], {}
    idx = lambda c: _off4(c["gidx"].to(torch.int32))  # noqa: E731
    pts_sites = ["points", "grid_idx"]
    # gather: a list of three planes, then a flat tensor
    for name in ("triplane_c16", "voxel_c32_flat"):
        c = GC.case(name)
        flat = c["form"] == "flat"
        grid = _off4(torch.cat([g.reshape(-1, g.shape[-1]) for g in c["grids"]]), True) if flat else [_off4(g, True) for g in c["grids"]]
        out = lp.sample_grid_at_points(_off4(c["pts"], True), grid, idx(c), grid_sizes=c["sizes"] if flat else None)
        out.backward(_off4(torch.randn(out.shape)))
        fields = ["grid.data"] if flat else [f"grid.grids[{k}].data" for k in range(3)]
        sites += [(e, f) for e in ("lp_point_gather", "lp_point_grad_points") for f in fields + pts_sites]
        sites += [(e, "vectors") for e in ("lp_point_grad_points", "lp_point_splat")] + [("lp_point_splat", f) for f in pts_sites]
    # splat: raw (differentiable in the points too), then normalised; the upstream grids reach the gather and the point gradient
    c = GC.case("triplane_c16")
    for normalize in (False, True):
        outs = lp.splat_points(_off4(c["pts"], not normalize), _off4(c["vec"], True), c["sizes"], idx(c), normalize=normalize)
        torch.autograd.backward(outs, [_off4(torch.randn(o.shape)) for o in outs])
    sites += [(e, f) for e in ("lp_point_splat", "lp_point_normalize") for f in pts_sites + ["vectors"]]
    # the decoder at points: two-grid decoder (a colour grid-list), a scaffold; the grids are AS_IS
    c = PC.case("voxel_c32_twogrid_022x32")
    d = c["dec"]
    dec = lp.DecoderParams(_off4(d.mlp_params, True), d.n_hidden_trunk, d.n_hidden_opacity, d.n_hidden_color, d.color_chn)
    grid, cgrid = [_off4(g, True) for g in c["grids"]], [_off4(g, True) for g in c["cgrids"]]
    scaffold = _off4((torch.rand(2, 3, 4, 5) < 0.6).float())
    op, col = lp.lightplane_eval_mlp(_off4(c["pts"], True), grid, idx(c), dec, _off4(c["enc"], True), PC.GAIN, scaffold=scaffold, color_grid=cgrid)
    torch.autograd.backward([op, col], [_off4(torch.randn(op.shape)), _off4(torch.randn(col.shape))])
    fwd, bwd = "lp_points_forward", "lp_points_backward"
    sites += [(e, f) for e in (fwd, bwd) for f in pts_sites + ["mlp_params", "encoding", "scaffold"]]
    sites += [(bwd, "grad_opacity"), (bwd, "grad_color")]
    for e in (fwd, bwd):
        as_is[(e, "grid.grids[0].data")] = [grid[0].data_ptr()]
        as_is[(e, "color_grid.grids[0].data")] = [cgrid[0].data_ptr()]
    # ... opacity only, a flat grid
    c = PC.case("triplane_c20_222x33_scaffold")
    d = c["dec"]
    dec = lp.DecoderParams(_off4(d.mlp_params, True), d.n_hidden_trunk, d.n_hidden_opacity, d.n_hidden_color, d.color_chn)
    flat = _off4(torch.cat([g.reshape(-1, g.shape[-1]) for g in c["grids"]]), True)
    op = lp.lightplane_eval_mlp_opacity_only(_off4(c["pts"], True), flat, idx(c), dec, PC.GAIN, scaffold=_off4(c["scaffold"]),
                                             grid_sizes=[list(g.shape) for g in c["grids"]])
    op.backward(_off4(torch.randn(op.shape)))
    for e in (fwd, bwd):
        as_is[(e, "grid.data")] = [flat.data_ptr()]
    # the ray clip: out of place, then in place on the rays' own near / far
    c = RC.case("random_2x5x6x7")
    clip = "lp_rays_clip"

    def rays():
        return lp.Rays(directions=_off4(c["d"]), origins=_off4(c["o"]), grid_idx=_off4(c["grid_idx"]), near=_off4(c["near"]), far=_off4(c["far"]))

    first = rays()  # (kept alive: the in-place call's tensors must not reuse its addresses)
    lp.clip_rays_to_scaffold(first, _off4(c["scaffold"]))
    sites += [(clip, f) for f in ("rays.directions", "rays.origins", "rays.grid_idx", "rays.near_t", "rays.far_t", "scaffold")]
    r = rays()
    lp.clip_rays_to_scaffold(r, _off4(c["scaffold"]), out=(r.near, r.far, torch.empty(r.near.shape[0], dtype=torch.uint8)))
    for f, t in (("near_out", r.near), ("rays.near_t", r.near), ("far_out", r.far), ("rays.far_t", r.far)):
        as_is[(clip, f)] = [t.data_ptr()]
    assert first.near.data_ptr() != r.near.data_ptr() and first.far.data_ptr() != r.far.data_ptr()
    return sites, as_is


def _run(drive):
    """(sites, AS_IS pointers) of a drive; the drives of the first four front-ends have no AS_IS input"""
    got = drive()
    sites, as_is = got if isinstance(got, tuple) else (got, {})
    for (entry, path), ptrs in as_is.items():
        assert _as_is_rule(entry, path), f"{entry}: {path} is not listed in AS_IS"
        assert all(p % 16 == 4 for p in ptrs), "the drive's AS_IS tensors sit at a 4-byte aligned base as well"
    return sites, as_is


def _split_as_is(seen, as_is):
    """(the record without the AS_IS pointers, the AS_IS pointers found): an AS_IS pointer is one the drive named, at its field"""
    found = [(k, p) for k, p in seen if p in as_is.get(k, ())]
    rest = [(k, p) for k, p in seen if p not in as_is.get(k, ())]
    missing = {k: [hex(p) for p in ptrs] for k, ptrs in as_is.items() if not set(ptrs) <= {p for kk, p in found if kk == k}}
    assert not missing, f"AS_IS inputs that did not arrive as the caller's pointer (copied?): {missing}"
    return rest, found


DRIVES = pytest.mark.parametrize("drive", [_drive_every_wrapper, _drive_mlp_splatter_and_embedding, _drive_the_modular_march,
                                           _drive_the_point_ops],
                                 ids=["renderer_splatter", "mlp_splatter_embedding", "modular_march", "point_ops"])


@pytest.mark.filterwarnings("ignore:lightplane_amd")
@DRIVES
def test_every_pointer_of_an_off4_input_arrives_aligned(recorder, drive):
    """With the helper in place no pointer of any recorded call is under-aligned: a helper call dropped at any site shows here.  (The
    AS_IS inputs are the caller's pointer: the library's to refuse.)"""
    sites, as_is = _run(drive)
    ptrs = recorder.pointers()
    seen, _ = _split_as_is(recorder.all_pointers(), as_is)
    bad = {k: hex(p) for k, p in seen if p % 16}
    assert not bad, f"under-aligned pointers reached the library: {bad}"
    for s in sites:
        assert s in ptrs, f"{s} was never handed to the library"


@pytest.mark.filterwarnings("ignore:lightplane_amd")
@DRIVES
def test_without_the_helper_every_input_pointer_arrives_under_aligned(recorder, monkeypatch, drive):
    """``_lib.aligned`` -> identity: EVERY pointer of every recorded call that is not a buffer the wrappers allocate themselves is the
    caller's, 4 bytes past a 16-byte boundary -- the expected set is derived from the record, not listed by hand.  Nothing else
    (``.contiguous()``, a dtype conversion, autograd) realigns an input, so the helper call at each site is load-bearing.  (The AS_IS
    inputs are the caller's pointer here as well.)"""
    monkeypatch.setattr(_lib, "aligned", lambda t, grid=False: t)
    sites, as_is = _run(drive)
    seen, _ = _split_as_is(recorder.all_pointers(), as_is)
    inputs = [(k, p) for k, p in seen if _is_input(*k)]
    own = [(k, p) for k, p in seen if not _is_input(*k)]
    assert inputs and own
    wrong = {k: hex(p) for k, p in inputs if p % 16 != 4}
    assert not wrong, f"input pointers that are not the caller's under-aligned ones: {wrong}"
    wrong = {k: hex(p) for k, p in own if p % 16}
    assert not wrong, f"buffers of the wrappers' own that are under-aligned: {wrong}"
    ptrs = dict(inputs)
    for s in sites:
        assert s in ptrs, f"{s} was never handed to the library as an input"

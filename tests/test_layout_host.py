"""CPU tests of the memory-layout contract (no GPU, no kernel launch).

* The C ABI refuses every device pointer that is not 16-byte aligned (include/lightplane_hip.h, Conventions) -- every pointer field of
  the three argument blocks, found from the ctypes struct definitions, on every entry point, before anything touches the device
  (fake pointers, ``n_rays == 0``).
* ``_lib.aligned``: the Python front-end's answer -- an aligned tensor passes through, a dense view at an element offset into a larger
  buffer is copied; the copy of a grid warns once per process.
* Mutation proof: with ``lib()`` replaced by a recorder, every pointer the wrappers hand over for inputs at a 4-byte aligned base is
  16-byte aligned, and with ``_lib.aligned`` replaced by the identity every one of those call sites hands over the under-aligned
  pointer -- the helper alone stands between such an input and the kernels, and a dropped call is noticed.
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
    got = {st.__name__: [p for p, _, _ in pointer_fields(st())] for st in (_lib.LpRays, _lib.LpGridList, _lib.LpRendererArgs,
                                                                         _lib.LpSplatterArgs, _lib.LpRayEmbedArgs)}
    assert got["LpRays"] == ["directions", "origins", "grid_idx", "near_t", "far_t", "encoding"]
    assert len(got["LpGridList"]) == 1 + _lib.LP_MAX_GRIDS
    # LpRendererArgs: rays 6, two grid-lists 2 x 9, scaffold + scaffold_shape.data, mlp_params, 3 outputs, ckpt, 3 upstream grads,
    # 4 flat gradient buffers, 2 x 8 list entries, bg_color, alpha, grad_alpha, seg_prefix
    assert len(got["LpRendererArgs"]) == 6 + 18 + 2 + 1 + 3 + 1 + 3 + 4 + 16 + 4
    assert len(got["LpSplatterArgs"]) == 6 + 18 + 2 + 1 + 5 + 8
    assert len(got["LpRayEmbedArgs"]) == 7
    assert "grid.grids[7].data" in got["LpRendererArgs"] and "grad_color_grid_list[7]" in got["LpRendererArgs"]
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
_OWN_BY_ENTRY = {"lp_ray_embedding_forward": ("out",), "lp_ray_embedding_backward": ("grad_weight", "grad_bias"),
                 "lp_splatter_normalize": ("feature", "weight")}


def _is_input(entry, path):
    if entry in _OWN_BY_ENTRY:
        return path not in _OWN_BY_ENTRY[entry]
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


DRIVES = pytest.mark.parametrize("drive", [_drive_every_wrapper, _drive_mlp_splatter_and_embedding],
                                 ids=["renderer_splatter", "mlp_splatter_embedding"])


@pytest.mark.filterwarnings("ignore:lightplane_amd")
@DRIVES
def test_every_pointer_of_an_off4_input_arrives_aligned(recorder, drive):
    """With the helper in place no pointer of any recorded call is under-aligned: a helper call dropped at any site shows here."""
    sites = drive()
    ptrs = recorder.pointers()
    bad = {k: hex(p) for k, p in recorder.all_pointers() if p % 16}
    assert not bad, f"under-aligned pointers reached the library: {bad}"
    for s in sites:
        assert s in ptrs, f"{s} was never handed to the library"


@pytest.mark.filterwarnings("ignore:lightplane_amd")
@DRIVES
def test_without_the_helper_every_input_pointer_arrives_under_aligned(recorder, monkeypatch, drive):
    """``_lib.aligned`` -> identity: EVERY pointer of every recorded call that is not a buffer the wrappers allocate themselves is the
    caller's, 4 bytes past a 16-byte boundary -- the expected set is derived from the record, not listed by hand.  Nothing else
    (``.contiguous()``, a dtype conversion, autograd) realigns an input, so the helper call at each site is load-bearing."""
    monkeypatch.setattr(_lib, "aligned", lambda t, grid=False: t)
    sites = drive()
    seen = recorder.all_pointers()
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

"""The GPU marching cubes (lightplane_amd/mesh.py, csrc/lp_mesh.hip) against the fp64 oracle of tests/mesh_cases.py.

For every lattice: ``faces``, both offset arrays and the counts are BIT-EXACT against the oracle (the output order is part of the
contract), and the vertices are within 1e-6 absolute in scene units -- ``t`` carries about 3 ulp of fp32 and the affine map to
[-1, 1] a few more, at magnitude <= 1 (an edge of a two-point axis is 2 units long: 4 ulp of t are 5e-7 there); the oracle computes
in fp64 from the same fp32 lattice values.  Normals are checked on smooth fields only, within 1e-4 per component, no vertex excluded.
Oracles are computed once per lattice and never modified.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import modules
from tests import mesh_cases as M
from tests.guarded_alloc import PATTERNS, guarded
from tests.layouts import make_layout
from tests.synth import RENDERER_CASES
from tests.test_gpu_parity import _dev

pytestmark = pytest.mark.gpu

VERTEX_TOL = 1e-6
NORMAL_TOL = 1e-4
_CACHE = {}


def _lattice(name):
    """(float32 lattice, level, oracle with normals) of a named case, computed once"""
    if name not in _CACHE:
        level = 0.0
        if name == "single":
            vol = M.single_cell_cases()
        elif name.startswith("two"):
            vol = M.two_cell_cases(int(name[-1]))
        elif name.startswith("noise"):
            k = int(name[-1])
            vol = M.padded_noise(M.NOISE_SHAPES[k], seed=k)
        elif name == "mid":
            vol = M.padded_noise(M.MID_SHAPE, seed=7)
        elif name == "deep":
            vol = M.sparse_blobs(M.DEEP_SHAPE)
        elif name == "sphere":
            vol = M.sphere(24)
        elif name == "sphere_box":
            vol, level = M.sphere(0, radius=0.7, size=(17, 24, 21)), 0.05
        elif name == "sines":
            vol, level = M.sin_product((13, 11, 17), batch=2), 0.1
        else:
            raise KeyError(name)
        _CACHE[name] = (vol, level, M.marching_cubes(vol, level, with_normals=True))
    return _CACHE[name]


def _np(mesh):
    return M.OracleMesh(mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy(), None if mesh.normals is None else mesh.normals.cpu().numpy(),
                        mesh.vertex_offsets.cpu().numpy(), mesh.face_offsets.cpu().numpy())


def _assert_mesh(got, ref, normals=False, what=""):
    assert got.vertex_offsets.dtype == np.int64 and got.face_offsets.dtype == np.int64 and got.faces.dtype == np.int32
    assert got.vertices.dtype == np.float32
    assert np.array_equal(got.vertex_offsets, ref.vertex_offsets), what
    assert np.array_equal(got.face_offsets, ref.face_offsets), what
    assert got.vertices.shape == ref.vertices.shape and got.faces.shape == ref.faces.shape, what
    assert np.array_equal(got.faces, ref.faces), what
    err = float(np.abs(got.vertices.astype(np.float64) - ref.vertices).max()) if ref.vertices.size else 0.0
    print(f"{what}: {ref.vertices.shape[0]} vertices, {ref.faces.shape[0]} faces, max vertex error {err:.3e}")
    assert err <= VERTEX_TOL, what
    if normals:
        nerr = float(np.abs(got.normals.astype(np.float64) - ref.normals).max())
        print(f"{what}: max normal error {nerr:.3e}")
        assert got.normals.shape == ref.normals.shape and nerr <= NORMAL_TOL, what


def _run(name, **kw):
    vol, level, ref = _lattice(name)
    mesh = lp.marching_cubes(torch.from_numpy(vol).to(_dev()), level, **kw)
    return _np(mesh), ref


# ---- exhaustive cases -----------------------------------------------------------------------------------------------------------------
def test_all_single_cell_cases():
    got, ref = _run("single")
    assert ref.faces.shape[0] == 820
    _assert_mesh(got, ref, what="256 single cells")


@pytest.mark.parametrize("axis", (0, 1, 2))
def test_all_two_cell_cases(axis):
    got, ref = _run(f"two{axis}")
    _assert_mesh(got, ref, what=f"4096 cell pairs across axis {axis}")
    for v, f in M.scenes(got):
        assert M.closed_and_oriented(f, v.shape[0])


# ---- random lattices and the scan hierarchy ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("noise0", "noise1", "mid"))
def test_noise_lattices(name):
    got, ref = _run(name)
    assert ref.faces.shape[0] > 0
    _assert_mesh(got, ref, what=name)
    for v, f in M.scenes(got):  # the kernel's own output, not the oracle's
        assert f.shape[0] > 0 and M.closed_and_oriented(f, v.shape[0]) and M.signed_volume(v, f) > 0.0


def test_lattice_beyond_every_scan_level():
    vol, _, ref = _lattice("deep")
    assert M.scan_levels(vol.size) == 3 and vol.size > M.SCAN_THRESHOLDS[-1]
    got, _ = _run("deep", with_normals=False)
    last = np.flatnonzero(vol.reshape(-1) > -1.0)[-1]
    assert last > vol.size - 3 * vol.shape[2] * vol.shape[3]  # a blob in the last tiles: its offsets carry every level's sums
    _assert_mesh(got, ref, what="deep")
    for v, f in M.scenes(got):  # (the blobs keep one layer away from the border: the kernel's own output is closed)
        assert f.shape[0] > 0 and M.closed_and_oriented(f, v.shape[0]) and M.signed_volume(v, f) > 0.0


# ---- normals --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("sphere", "sphere_box", "sines"))
def test_normals_on_smooth_fields(name):
    got, ref = _run(name, with_normals=True)
    assert ref.vertices.shape[0] > 100
    _assert_mesh(got, ref, normals=True, what=name)
    length = np.linalg.norm(got.normals.astype(np.float64), axis=1)
    assert np.abs(length - 1.0).max() <= 1e-6
    plain, _ = _run(name)
    assert plain.normals is None and np.array_equal(plain.vertices, got.vertices) and np.array_equal(plain.faces, got.faces)


def test_sphere_is_closed_with_the_measured_volume():
    got, _ = _run("sphere")
    V = got.vertices.shape[0]
    assert M.closed_and_oriented(got.faces, V) and M.euler_characteristic(got.faces, V) == 2
    want = 0.98765 * 4.0 / 3.0 * np.pi * 0.6 ** 3
    assert abs(M.signed_volume(got.vertices, got.faces) - want) <= 1e-4 * want


# ---- degenerate inputs ----------------------------------------------------------------------------------------------------------------
def _direct(vol, level, **kw):
    ref = M.marching_cubes(vol, level, with_normals=False)
    got = _np(lp.marching_cubes(torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float32)).to(_dev()), level, **kw))
    return got, ref


def test_values_equal_to_the_level():
    rng = np.random.default_rng(5)
    vol = rng.integers(-1, 2, size=(2, 6, 5, 7)).astype(np.float32) * 0.5       # a third of the points sit exactly on the level
    for level in (0.0, 0.5, -0.5):      # (at -0.5 every point is inside, >=: the mesh is empty)
        got, ref = _direct(vol, level)
        assert (ref.faces.shape[0] > 0) == (level > -0.5)
        _assert_mesh(got, ref, what=f"values on the level {level}")


def test_nan_and_infinite_entries():
    vol = M.padded_noise((2, 7, 6, 8), seed=9)
    rng = np.random.default_rng(6)
    idx = rng.choice(vol.size, 60, replace=False)
    flat = vol.reshape(-1)
    flat[idx[:20]], flat[idx[20:40]], flat[idx[40:]] = np.nan, np.inf, -np.inf
    got, ref = _direct(vol, 0.0)
    assert np.isfinite(got.vertices).all()
    _assert_mesh(got, ref, what="NaN / inf entries")
    all_nan, ref_nan = _direct(np.full((1, 3, 3, 3), np.nan, np.float32), 0.0)
    _assert_mesh(all_nan, ref_nan, what="all NaN")
    assert all_nan.faces.shape[0] == 0


def test_finite_values_whose_difference_overflows():
    big = np.float32(3e38)
    vol = np.full((1, 4, 5, 6), -big, np.float32)
    vol[0, 1:3, 1:4, 1:5] = big                                  # v_hi - v_lo = 6e38 is not an fp32 number; t is 0.5 all the same
    vol[0, 1, 1, 1], vol[0, 2, 3, 4] = np.float32(1e38), np.float32(2.5e38)
    for level in (0.0, 1e30, -2e38):
        got, ref = _direct(vol, level)
        assert ref.faces.shape[0] > 0
        _assert_mesh(got, ref, what=f"+-3e38 at level {level:g}")
        assert M.closed_and_oriented(got.faces, got.vertices.shape[0])


def test_constant_volume_and_singleton_axes():
    for vol, level in ((np.full((2, 4, 5, 6), 0.25, np.float32), 0.25), (np.full((2, 4, 5, 6), 0.25, np.float32), 0.3),
                       (M.noise((2, 1, 5, 6)), 0.0), (M.noise((2, 5, 1, 6)), 0.0), (M.noise((2, 5, 6, 1)), 0.0), (M.noise((1, 1, 1, 1)), 0.0)):
        got, ref = _direct(vol, level, with_normals=True)
        assert got.vertices.shape == (0, 3) and got.faces.shape == (0, 3) and got.normals.shape == (0, 3)
        assert not got.vertex_offsets.any() and not got.face_offsets.any()
        assert got.vertex_offsets.shape == (vol.shape[0] + 1,)
        _assert_mesh(got, ref, what=f"empty {vol.shape}")


def test_batch_of_empty_and_non_empty_scenes():
    vol = np.full((5, 6, 7, 5), -1.0, np.float32)
    vol[1], vol[3] = M.padded_noise((1, 6, 7, 5), seed=2)[0], M.sphere(0, radius=0.5, size=(6, 7, 5))[0]
    got, ref = _direct(vol, 0.0)
    counts = np.diff(ref.face_offsets)
    assert counts[0] == counts[2] == counts[4] == 0 and counts[1] > 0 and counts[3] > 0
    _assert_mesh(got, ref, what="mixed batch")
    one, ref3 = _direct(vol[3], 0.0)                         # a [D, H, W] volume is a batch of one
    _assert_mesh(one, ref3, what="3-D volume")
    lo, hi = ref.face_offsets[3], ref.face_offsets[4]
    assert np.array_equal(one.faces, got.faces[lo:hi])       # vertex ids are local to the scene


# ---- capacity mode --------------------------------------------------------------------------------------------------------------------
def _assert_written(g, rec, ref_values, n, tol, what):
    """Element by element: nothing below row ``n`` still holds the poison, everything from row ``n`` on does.  One exemption, under the
    plausible pattern 0.5 and for float buffers only: an element whose fp64 oracle value is 0.5 to within the buffer's tolerance -- only
    there may a correct kernel write the very value of the poison (the caller compares every value with the oracle as well, so an
    unwritten 0.5 anywhere else fails twice)."""
    unwritten = g.unwritten_mask(rec).reshape(-1, 3).cpu().numpy()
    allowed = np.zeros(unwritten[:n].shape, dtype=bool)
    if rec.pattern == "0.5" and rec.dtype == torch.float32:
        allowed = np.abs(np.asarray(ref_values[:n], dtype=np.float64) - 0.5) <= tol
    assert not (unwritten[:n] & ~allowed).any(), f"{what}: an element below the count was not written"
    assert unwritten[n:].all(), f"{what}: an element at or beyond the count was written"


def _assert_values(mesh, ref, n_v, n_f, what):
    """the first n_v vertices / normals and n_f faces of a GPU result against the oracle"""
    assert np.array_equal(mesh.faces[:n_f].cpu().numpy(), ref.faces[:n_f]), what
    if n_v:
        assert np.abs(mesh.vertices[:n_v].cpu().numpy().astype(np.float64) - ref.vertices[:n_v]).max() <= VERTEX_TOL, what
        assert np.abs(mesh.normals[:n_v].cpu().numpy().astype(np.float64) - ref.normals[:n_v]).max() <= NORMAL_TOL, what


# (the poison tests run on the smooth two-scene sine lattice, where the normals are held to the oracle as well)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_capacity_mode_under_poison_and_fences(pattern):
    vol, level, ref = _lattice("sines")
    V, F = ref.vertices.shape[0], ref.faces.shape[0]
    dvol = torch.from_numpy(vol).to(_dev())
    for cap_v, cap_f in ((V + 37, F + 11), (V, F), (V - 29, F - 13), (0, 0)):
        what = f"{pattern}, capacities ({cap_v}, {cap_f})"
        n_v, n_f = min(V, cap_v), min(F, cap_f)
        with guarded(pattern) as g:
            mesh = lp.marching_cubes(dvol, level, with_normals=True, max_vertices=cap_v, max_faces=cap_f)
            torch.cuda.synchronize()
            recs = {r.name: r for r in g.from_file("lightplane_amd/mesh.py")}
            assert {"vertices", "faces", "normals", "vertex_offsets", "face_offsets", "workspace"} <= set(recs), sorted(recs)
            # the counts report the true need, whatever the capacity
            assert np.array_equal(mesh.vertex_offsets.cpu().numpy(), ref.vertex_offsets)
            assert np.array_equal(mesh.face_offsets.cpu().numpy(), ref.face_offsets)
            assert mesh.vertices.shape == (cap_v, 3) and mesh.faces.shape == (cap_f, 3) and mesh.normals.shape == (cap_v, 3)
            if cap_v:
                _assert_written(g, recs["vertices"], ref.vertices, n_v, VERTEX_TOL, f"vertices, {what}")
                _assert_written(g, recs["normals"], ref.normals, n_v, NORMAL_TOL, f"normals, {what}")
            if cap_f:
                _assert_written(g, recs["faces"], ref.faces, n_f, 0.0, f"faces, {what}")
            assert g.unwritten(recs["vertex_offsets"]) == 0 and g.unwritten(recs["face_offsets"]) == 0
        # (leaving the block checked every fence)
        _assert_values(mesh, ref, n_v, n_f, what)


def test_default_mode_writes_every_element():
    vol, level, ref = _lattice("sines")
    V, F = ref.vertices.shape[0], ref.faces.shape[0]
    dvol = torch.from_numpy(vol).to(_dev())
    for pattern in PATTERNS:
        with guarded(pattern) as g:
            mesh = lp.marching_cubes(dvol, level, with_normals=True)
            torch.cuda.synchronize()
            recs = {r.name: r for r in g.from_file("lightplane_amd/mesh.py")}
            assert mesh.vertices.shape == (V, 3) and mesh.faces.shape == (F, 3) and mesh.normals.shape == (V, 3)
            _assert_written(g, recs["vertices"], ref.vertices, V, VERTEX_TOL, f"vertices, {pattern}")
            _assert_written(g, recs["normals"], ref.normals, V, NORMAL_TOL, f"normals, {pattern}")
            _assert_written(g, recs["faces"], ref.faces, F, 0.0, f"faces, {pattern}")
            assert g.unwritten(recs["vertex_offsets"]) == 0 and g.unwritten(recs["face_offsets"]) == 0
        _assert_mesh(_np(mesh), ref, normals=True, what=f"default mode under {pattern}")


def test_graph_capture_and_replay():
    dev = _dev()
    vol, level, ref = _lattice("noise0")
    other = M.padded_noise(M.NOISE_SHAPES[0], seed=5)
    ref_other = M.marching_cubes(other, level)
    cap_v = max(ref.vertices.shape[0], ref_other.vertices.shape[0]) + 5
    cap_f = max(ref.faces.shape[0], ref_other.faces.shape[0]) + 5
    dvol = torch.from_numpy(vol).to(dev)
    ws = torch.empty(lp.mesh_workspace_bytes(vol.shape), dtype=torch.uint8, device=dev)
    kw = dict(with_normals=True, max_vertices=cap_v, max_faces=cap_f, workspace=ws)
    eager = lp.marching_cubes(dvol, level, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lp.marching_cubes(dvol, level, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = lp.marching_cubes(dvol, level, **kw)
    for t in (res.vertices, res.faces, res.normals):
        t.fill_(7)
    res.vertex_offsets.fill_(-5)
    res.face_offsets.fill_(-5)
    graph.replay()
    torch.cuda.synchronize()
    n_v, n_f = ref.vertices.shape[0], ref.faces.shape[0]
    assert torch.equal(res.vertex_offsets, eager.vertex_offsets) and torch.equal(res.face_offsets, eager.face_offsets)
    assert int(res.vertex_offsets[-1]) == n_v and int(res.face_offsets[-1]) == n_f
    assert torch.equal(res.vertices[:n_v], eager.vertices[:n_v]) and torch.equal(res.faces[:n_f], eager.faces[:n_f])
    assert torch.equal(res.normals[:n_v], eager.normals[:n_v])
    assert bool((res.vertices[n_v:] == 7).all()) and bool((res.faces[n_f:] == 7).all())
    dvol.copy_(torch.from_numpy(other))  # new values in the tensor the graph reads
    graph.replay()
    torch.cuda.synchronize()
    n_v, n_f = ref_other.vertices.shape[0], ref_other.faces.shape[0]
    assert np.array_equal(res.face_offsets.cpu().numpy(), ref_other.face_offsets)
    assert np.array_equal(res.faces[:n_f].cpu().numpy(), ref_other.faces)
    assert np.abs(res.vertices[:n_v].cpu().numpy().astype(np.float64) - ref_other.vertices).max() <= VERTEX_TOL


def test_results_are_bit_reproducible():
    vol, level, _ = _lattice("noise1")
    dvol = torch.from_numpy(vol).to(_dev())
    a, b = lp.marching_cubes(dvol, level, with_normals=True), lp.marching_cubes(dvol, level, with_normals=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---- layouts --------------------------------------------------------------------------------------------------------------------------
def test_layouts_are_refused():
    dev = _dev()
    vol, level, ref = _lattice("noise0")
    values = torch.from_numpy(vol)
    _, view = make_layout(values, "strided", kind="grid").on(dev)
    assert not view.is_contiguous()
    with pytest.raises(AssertionError, match="must be contiguous"):
        lp.marching_cubes(view, level)
    _, view = make_layout(values, "off4").on(dev)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    with pytest.raises(AssertionError, match=r"volume = 0x[0-9a-f]+ has to be 16-byte aligned"):
        lp.marching_cubes(view, level)
    _, view = make_layout(values, "off8").on(dev)
    with pytest.raises(AssertionError, match="has to be 16-byte aligned"):
        lp.marching_cubes(view, level)
    # an offset of four elements is aligned and goes through as it is
    buf = torch.randn(values.numel() + 8, device=dev)
    view = buf[4:4 + values.numel()].view(values.shape)
    view.copy_(values)
    _assert_mesh(_np(lp.marching_cubes(view, level)), ref, what="view at a 16-byte offset")
    with pytest.raises(AssertionError, match="workspace has to be"):
        lp.marching_cubes(values.to(dev), level, workspace=torch.empty(16, dtype=torch.uint8, device=dev))


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def _decoder_on(dec, dev):
    return lp.DecoderParams(dec.mlp_params.to(dev), dec.n_hidden_trunk, dec.n_hidden_opacity, dec.n_hidden_color, dec.color_chn)


@pytest.mark.parametrize("case", ("triplane_basic", "voxel_basic"))
def test_extract_mesh_is_scaffold_opacity_then_marching_cubes(case):
    dev = _dev()
    d = next(c for c in RENDERER_CASES if c.name == case).build()
    grids, dec = [g.to(dev) for g in d["grids"]], _decoder_on(d["decoder"], dev)
    B = grids[0].shape[0]
    size = [B, 13, 11, 15]
    gain = 1.3
    opacity = lp.scaffold_opacity(grids, dec, size, gain=gain)
    level = float(opacity.median())
    want = lp.marching_cubes(opacity, level, with_normals=True)
    assert want.faces.shape[0] > 50
    enc = torch.randn(B, int(dec.n_hidden_color[0]), generator=torch.Generator().manual_seed(3)).to(dev)
    got = lp.extract_mesh(grids, dec, size, level=level, gain=gain, rays_encoding=enc)
    for name in ("vertices", "faces", "normals", "vertex_offsets", "face_offsets"):
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    bounds = got.vertex_offsets.tolist()
    assert got.colors.shape == (bounds[-1], dec.color_chn)
    for b in range(B):
        lo, hi = bounds[b], bounds[b + 1]
        assert hi > lo
        _, col = lp.lightplane_eval_mlp(got.vertices[lo:hi][None], grids, torch.full((1,), b, dtype=torch.int32, device=dev), dec,
                                        enc[b:b + 1], gain)
        assert torch.equal(got.colors[lo:hi], col[0]), f"colours of scene {b}"
    plain = lp.extract_mesh(grids, dec, size, level=level, gain=gain, with_normals=False)
    assert plain.colors is None and plain.normals is None and torch.equal(plain.faces, want.faces)
    # flat form of the same grid-list
    C = grids[0].shape[-1]
    flat = torch.cat([g.reshape(-1, C) for g in grids])
    got_flat = lp.extract_mesh(flat, dec, size, level=level, gain=gain, grid_sizes=[list(g.shape) for g in grids], rays_encoding=enc)
    assert torch.equal(got_flat.vertices, got.vertices) and torch.equal(got_flat.colors, got.colors)


def test_module_method_calls_the_fused_path(monkeypatch):
    dev = _dev()
    torch.manual_seed(0)
    renderer = lp.LightplaneRenderer(num_samples=8, color_chn=3, grid_chn=16, mlp_hidden_chn=32, gain=2.0).to(dev)
    gen = torch.Generator().manual_seed(4)
    grids = [torch.randn(2, *s, 16, generator=gen).to(dev) for s in ((1, 6, 7), (5, 1, 7), (5, 6, 1))]
    size = [2, 9, 10, 11]
    dec = renderer.get_decoder_params()
    opacity = lp.scaffold_opacity(grids, dec, size, gain=2.0, mask_out_of_bounds_samples=renderer.mask_out_of_bounds_samples)
    level = float(opacity.median())
    calls = []
    real = modules._fused_extract_mesh

    def spy(*args, **kwargs):
        calls.append(kwargs)
        return real(*args, **kwargs)

    monkeypatch.setattr(modules, "_fused_extract_mesh", spy)
    dirs = torch.tensor([[0.0, 0.0, -1.0], [1.0, 0.0, 0.0]], device=dev)
    mesh = renderer.extract_mesh(grids, size, level=level, view_directions=dirs)
    assert len(calls) == 1 and calls[0]["gain"] == 2.0 and calls[0]["level"] == level
    want = lp.marching_cubes(opacity, level, with_normals=True)
    assert torch.equal(mesh.vertices, want.vertices) and torch.equal(mesh.faces, want.faces) and torch.equal(mesh.normals, want.normals)
    assert mesh.colors.shape == (mesh.vertices.shape[0], 3) and float(mesh.colors.min()) >= 0.0 and float(mesh.colors.max()) <= 1.0
    assert renderer.extract_mesh(grids, size, level=level, with_normals=False).colors is None


def _read_ply(path):
    with open(path) as f:
        lines = f.read().split("\n")
    end = lines.index("end_header")
    head = lines[:end]
    assert head[0] == "ply" and head[1] == "format ascii 1.0"
    n_v = int(next(h for h in head if h.startswith("element vertex")).split()[-1])
    n_f = int(next(h for h in head if h.startswith("element face")).split()[-1])
    body = [l for l in lines[end + 1:] if l]
    assert len(body) == n_v + n_f
    verts = np.array([[float(v) for v in l.split()] for l in body[:n_v]]).reshape(n_v, 9)
    faces = np.array([[int(v) for v in l.split()] for l in body[n_v:]], dtype=np.int64).reshape(n_f, 4)
    return verts, faces


def test_fit_synthetic_scene_exports_a_mesh(tmp_path):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("fit_synthetic_scene", os.path.join(repo, "examples", "fit_synthetic_scene.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    path = str(tmp_path / "ball.ply")
    old = lp.config.stop_transmittance
    try:
        r = mod.main(["--steps", "60", "--rays", "2048", "--res", "16", "--export-mesh", path, "--mesh-size", "24", "--mesh-level", "1.0"])
    finally:
        lp.config.stop_transmittance = old
    print("fit with a mesh:", r)
    assert r["mesh_file"] == path and r["mesh_vertices"] > 0 and r["mesh_faces"] > 0
    verts, faces = _read_ply(path)
    assert verts.shape[0] == r["mesh_vertices"] and faces.shape[0] == r["mesh_faces"]
    assert (faces[:, 0] == 3).all() and faces[:, 1:].min() >= 0 and faces[:, 1:].max() < verts.shape[0]
    assert np.isfinite(verts).all() and np.abs(verts[:, :3]).max() <= 1.0
    assert verts[:, 6:].min() >= 0 and verts[:, 6:].max() <= 255
    assert M.closed_and_oriented(faces[:, 1:], verts.shape[0])          # the ball does not reach the lattice border
    assert M.signed_volume(verts[:, :3], faces[:, 1:]) > 0.0

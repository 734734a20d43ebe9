"""CPU tests of the mesh extraction: the generated marching-cubes table (scripts/gen_mc_table.py, csrc/lp_mc_table.h), the fp64 oracle
and the scan ledger of tests/mesh_cases.py, the lp_mesh_* symbols and the ABI struct, and every argument check of the entry points
(each returns its code and message before anything touches a device)."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import lightplane_amd as lp
from lightplane_amd import _lib, mesh
from tests import mesh_cases as M

GEN = M.GEN
FAKE = 0x10000     # 16-byte-aligned non-NULL "device pointers": no check dereferences them, and every call below fails a check
STEP = 0x1000000


# ---- the table ------------------------------------------------------------------------------------------------------------------------
def test_committed_header_is_what_the_generator_emits():
    assert open(M.HEADER).read() == GEN.emit(), "lightplane_amd/csrc/lp_mc_table.h is stale: python scripts/gen_mc_table.py --write"


def test_table_size():
    t = M.TABLE
    assert t.shape == (256, 16)
    assert int(t[:, 0].sum()) == 820 and int(t[:, 0].max()) == 5
    assert t[0, 0] == 0 and t[255, 0] == 0
    assert ((t[:, 1:] >= 0) & (t[:, 1:] < 12)).all()
    for c in range(256):
        assert (t[c, 1 + 3 * t[c, 0]:] == 0).all()          # nothing behind the last triangle
    assert GEN.EDGES == [(0, 1), (0, 2), (0, 4), (1, 3), (1, 5), (2, 3), (2, 6), (3, 7), (4, 5), (4, 6), (5, 7), (6, 7)]


def test_every_crossed_edge_has_one_predecessor_and_one_successor():
    for case in range(256):
        crossed = {e for e, (a, b) in enumerate(GEN.EDGES) if ((case >> a) ^ (case >> b)) & 1}
        segs = GEN.segments(case)
        assert sorted(a for a, _ in segs) == sorted(crossed), case
        assert sorted(b for _, b in segs) == sorted(crossed), case


def test_triangles_cover_the_contour_and_no_diagonal_lies_in_a_face():
    for case in range(256):
        row = M.TABLE[case]
        tris = [tuple(int(v) for v in row[1 + 3 * k: 4 + 3 * k]) for k in range(int(row[0]))]
        segs = set(GEN.segments(case))
        directed = [(t[k], t[(k + 1) % 3]) for t in tris for k in range(3)]
        assert len(set(directed)) == len(directed), case
        boundary = [d for d in directed if d in segs]
        assert sorted(boundary) == sorted(segs), case                       # every contour segment is the edge of one triangle
        for a, b in directed:
            if (a, b) in segs:
                continue
            assert (b, a) in directed, case                                  # a diagonal is shared by two triangles of the fan
            assert not GEN.edges_share_face(a, b), (case, a, b)


def test_faces_are_counter_clockwise_from_outside():
    for k, loop in enumerate(GEN.FACES):
        p = np.array([GEN.CORNERS[c] for c in loop], dtype=float)
        n = np.cross(p[1] - p[0], p[2] - p[1])
        want = np.zeros(3)
        want[k // 2] = 1.0 if k % 2 else -1.0
        assert np.array_equal(n, want), (k, loop)


# ---- the oracle -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", (0, 1, 2))
def test_two_cell_patterns_are_closed_and_oriented(axis):
    vol = M.two_cell_cases(axis)
    assert vol.shape == {0: (4096, 4, 4, 5), 1: (4096, 4, 5, 4), 2: (4096, 5, 4, 4)}[axis]
    m = M.marching_cubes(vol, 0.0)
    n_nonempty = 0
    for v, f in M.scenes(m):
        assert M.closed_and_oriented(f, v.shape[0])
        if f.shape[0]:
            n_nonempty += 1
            assert M.signed_volume(v, f) > 0.0
    assert n_nonempty == 4095


def test_single_cells_use_the_whole_table():
    m = M.marching_cubes(M.single_cell_cases(), 0.0)
    assert np.array_equal(np.diff(m.face_offsets), M.TABLE[:, 0])
    assert m.faces.shape[0] == 820
    crossed = [sum(((c >> a) ^ (c >> b)) & 1 for a, b in GEN.EDGES) for c in range(256)]
    assert np.array_equal(np.diff(m.vertex_offsets), crossed)


def test_sphere():
    m = M.marching_cubes(M.sphere(24), 0.0, with_normals=True)
    V = m.vertices.shape[0]
    assert M.closed_and_oriented(m.faces, V)
    assert M.euler_characteristic(m.faces, V) == 2
    want = 0.98765 * 4.0 / 3.0 * np.pi * 0.6 ** 3
    assert abs(M.signed_volume(m.vertices, m.faces) - want) <= 1e-4 * want
    radial = m.vertices / np.linalg.norm(m.vertices, axis=1, keepdims=True)
    assert ((m.normals * radial).sum(axis=1) > 0.999).all()       # -grad of (0.6 - |p|) points outwards


def test_padded_noise_is_closed():
    m = M.marching_cubes(M.padded_noise((1, 6, 6, 6), seed=3), 0.0)
    assert m.faces.shape[0] > 0 and M.closed_and_oriented(m.faces, m.vertices.shape[0])
    assert M.signed_volume(m.vertices, m.faces) > 0.0


def test_degenerate_lattices():
    for shape in ((2, 1, 5, 6), (2, 5, 1, 6), (2, 5, 6, 1), (1, 1, 1, 1)):
        m = M.marching_cubes(M.noise(shape), 0.0, with_normals=True)
        assert m.vertices.shape == (0, 3) and m.faces.shape == (0, 3) and not m.vertex_offsets.any() and not m.face_offsets.any()
    m = M.marching_cubes(np.full((2, 3, 4, 5), 0.25, np.float32), 0.25)      # everything inside (>=): no crossing
    assert m.vertices.shape[0] == 0 and m.faces.shape[0] == 0
    vol = M.padded_noise((1, 5, 5, 5), seed=1)
    vol[0, 2, 2, 2], vol[0, 2, 2, 3], vol[0, 1, 2, 2] = np.nan, np.inf, -np.inf
    m = M.marching_cubes(vol, 0.0, with_normals=True)
    assert np.isfinite(m.vertices).all() and M.closed_and_oriented(m.faces, m.vertices.shape[0])


# ---- the scan ledger ------------------------------------------------------------------------------------------------------------------
def test_gpu_lattices_cross_every_scan_threshold():
    assert M.SCAN_THRESHOLDS == (256, 65536, 16777216)
    points = {s: int(np.prod(s)) for s in M.NOISE_SHAPES + (M.MID_SHAPE, M.DEEP_SHAPE)}
    for k, limit in enumerate(M.SCAN_THRESHOLDS):
        assert any(n > limit for n in points.values()), f"no lattice of more than {limit} points"
    assert [M.scan_levels(n) for n in (1, 256, 257, 65536, 65537, 2 ** 24, 2 ** 24 + 1)] == [1, 1, 1, 1, 2, 2, 3]
    assert M.scan_levels(points[M.NOISE_SHAPES[0]]) == 1 and M.scan_levels(points[M.NOISE_SHAPES[1]]) == 1
    assert M.scan_levels(points[M.MID_SHAPE]) == 2 and M.scan_levels(points[M.DEEP_SHAPE]) == 3
    assert M.scan_levels(2 ** 31 - 1) == 3          # the top of the hierarchy for every lattice the library takes
    for s in M.NOISE_SHAPES:                        # odd sizes, no multiple of the tile
        assert all(v % 2 == 1 for v in s[1:]) and points[s] % M.MC_TILE != 0
    assert points[M.DEEP_SHAPE] % M.MC_TILE != 0 and points[M.MID_SHAPE] % M.MC_TILE != 0


def test_workspace_bytes_match_the_ledger():
    for shape in M.NOISE_SHAPES + (M.MID_SHAPE, M.DEEP_SHAPE, (1, 1, 1, 1), (3, 512, 512, 512), (256, 2, 2, 2), (1, 1, 1, 2 ** 31 - 1)):
        n = int(np.prod(shape))
        got = lp.mesh_workspace_bytes(shape)
        assert got == M.workspace_bytes(n), shape
        tiles = -(-n // M.MC_TILE)
        assert got <= 8 * n + 16 * (tiles + -(-tiles // M.MC_SCAN) + 256 + 1) + 16, shape     # <= 8 bytes per point + the tile sums
    assert lp.mesh_workspace_bytes((5, 6, 7)) == lp.mesh_workspace_bytes((1, 5, 6, 7))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def _args(shape=(2, 5, 6, 7)):
    a = _lib.LpMeshArgs()
    a.volume = FAKE
    a.shape = _lib.LpGrid(*shape, 0, None)
    a.level = 0.5
    a.vertex_offsets, a.face_offsets = FAKE + STEP, FAKE + 2 * STEP
    a.vertices, a.faces, a.normals = FAKE + 3 * STEP, FAKE + 4 * STEP, FAKE + 5 * STEP
    a.max_vertices, a.max_faces = 10, 10
    return a


def _err():
    return _lib.lib().lp_last_error().decode()


def _call(name, a, ws=FAKE + 6 * STEP, nbytes=None):
    L = _lib.lib()
    if nbytes is None:
        nbytes = L.lp_mesh_workspace_bytes(ctypes.byref(a))
    return getattr(L, name)(ctypes.byref(a), ws, nbytes, None)


def test_symbols_struct_and_exports():
    L = _lib.lib()
    for name in ("lp_mesh_workspace_bytes", "lp_mesh_count", "lp_mesh_emit"):
        assert hasattr(L, name), f"{name} not exported by liblightplane_hip.so"
    assert "lp_mesh_count" in _lib.EXPORTS and "lp_mesh_emit" in _lib.EXPORTS
    assert L.lp_abi_sizeof(16) == ctypes.sizeof(_lib.LpMeshArgs)
    for which in (15, 17, 99):
        assert L.lp_abi_sizeof(which) == -1, which
    assert L.lp_abi_sizeof(14) == ctypes.sizeof(_lib.LpPointGridArgs)
    assert L.lp_version() == 207  # additive: no version change
    info = _lib.build_info()
    assert set(info["mesh"]) == {"table", "count", "scan", "emit"}
    assert "point_grid" in info and "scaffold" in info
    for name in ("marching_cubes", "extract_mesh", "mesh_workspace_bytes"):
        assert name in lp.__all__ and getattr(lp, name) is getattr(mesh, name)
    assert hasattr(lp.LightplaneRenderer, "extract_mesh")


def test_signatures():
    sig = inspect.signature(lp.marching_cubes)
    assert list(sig.parameters) == ["volume", "level", "with_normals", "max_vertices", "max_faces", "workspace"]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for n, p in sig.parameters.items() if n not in ("volume", "level"))
    assert sig.parameters["with_normals"].default is False
    sig = inspect.signature(lp.extract_mesh)
    assert list(sig.parameters) == ["feature_grid", "decoder_params", "lattice_size", "level", "gain", "mask_out_of_bounds_samples",
                                    "grid_sizes", "with_normals", "rays_encoding", "color_grid", "color_grid_sizes"]
    assert sig.parameters["level"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["with_normals"].default is True
    assert mesh.Mesh._fields == ("vertices", "faces", "normals", "vertex_offsets", "face_offsets")


def test_null_arguments_are_refused():
    L = _lib.lib()
    assert L.lp_mesh_workspace_bytes(None) == -3 and "args is NULL" in _err()
    for name in ("lp_mesh_count", "lp_mesh_emit"):
        assert getattr(L, name)(None, FAKE, 1 << 20, None) == -3 and "args is NULL" in _err(), name
        a = _args()
        a.volume = None
        assert _call(name, a) == -3 and "volume is NULL" in _err(), name
        for field in ("vertex_offsets", "face_offsets"):
            a = _args()
            setattr(a, field, None)
            assert _call(name, a) == -3 and "vertex_offsets / face_offsets is NULL" in _err(), (name, field)
        assert _call(name, _args(), ws=None) == -3 and "workspace is NULL" in _err(), name
    for field, cap in (("vertices", "max_vertices"), ("faces", "max_faces")):
        a = _args()
        setattr(a, field, None)
        assert _call("lp_mesh_emit", a) == -3 and f"{field} is NULL" in _err()
        setattr(a, cap, 0)     # nothing to write: NULL is fine, and the next check fails
        assert _call("lp_mesh_emit", a, nbytes=1) == -1 and "workspace of 1 bytes" in _err()


def test_malformed_arguments_are_refused():
    L = _lib.lib()
    for shape in ((0, 5, 6, 7), (2, 0, 6, 7), (2, 5, -1, 7), (2, 5, 6, 0)):
        a = _args(shape)
        assert L.lp_mesh_workspace_bytes(ctypes.byref(a)) == -1 and "extent < 1" in _err(), shape
        for name in ("lp_mesh_count", "lp_mesh_emit"):
            assert _call(name, a, nbytes=1 << 20) == -1 and "extent < 1" in _err(), (name, shape)
    for shape in ((1, 2048, 1024, 1024), (2, 1024, 1024, 1024), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)):
        a = _args(shape)
        assert L.lp_mesh_workspace_bytes(ctypes.byref(a)) == -2 and "below 2^31" in _err(), shape
        assert _call("lp_mesh_count", a, nbytes=1 << 40) == -2 and "below 2^31" in _err(), shape
    assert L.lp_mesh_workspace_bytes(ctypes.byref(_args((1, 2047, 1024, 1024)))) > 0
    for name in ("lp_mesh_count", "lp_mesh_emit"):
        a = _args()
        need = L.lp_mesh_workspace_bytes(ctypes.byref(a))
        assert _call(name, a, nbytes=need - 1) == -1 and f"asks for {need}" in _err(), name
    for cap in ("max_vertices", "max_faces"):
        a = _args()
        setattr(a, cap, -1)
        assert _call("lp_mesh_emit", a) == -1 and "have to be >= 0" in _err()


def test_under_aligned_pointers_are_refused():
    for name in ("lp_mesh_count", "lp_mesh_emit"):
        for field in ("volume", "vertex_offsets", "face_offsets", "vertices", "faces", "normals"):
            for off in (4, 8):
                a = _args()
                setattr(a, field, getattr(a, field) + off)
                assert _call(name, a) == -1, (name, field)
                assert _err().startswith(f"{field} = ") and "has to be 16-byte aligned" in _err(), _err()
        assert _call(name, _args(), ws=FAKE + 6 * STEP + 8) == -1 and _err().startswith("workspace = "), name


def test_wrappers_check_their_inputs():
    with pytest.raises(AssertionError, match="max_vertices and max_faces go together"):
        lp.marching_cubes(torch.zeros(2, 3, 4, 5), 0.0, max_vertices=3)
    with pytest.raises(AssertionError, match="volume has to be"):
        lp.marching_cubes(torch.zeros(3, 4), 0.0)
    with pytest.raises(AssertionError, match="float32"):
        lp.marching_cubes(torch.zeros(2, 3, 4, 5, dtype=torch.float64), 0.0)
    with pytest.raises(_lib.LightplaneHipError, match="GPU only"):
        lp.marching_cubes(torch.zeros(2, 3, 4, 5), 0.0)      # there is no CPU path
    with pytest.raises(AssertionError, match="positive"):
        lp.mesh_workspace_bytes((2, 0, 4, 5))

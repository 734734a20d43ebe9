"""The lattices of the mesh tests and their fp64 oracle: a vectorised numpy marching cubes over the generated table
(scripts/gen_mc_table.py), with the ordering contract of lightplane_amd/mesh.py (tests/test_mesh_host.py checks the table, the oracle
and this ledger without a GPU; tests/test_gpu_mesh.py holds the kernels of csrc/lp_mesh.hip to the oracle).

Contract (include/lightplane_hip.h, LpMeshArgs): lattice point n = ((b D + z) H + y) W + x at (lin(W)[x], lin(H)[y], lin(D)[z]); inside =
``value >= level`` in fp32 (a NaN is outside); a lattice edge belongs to its lower endpoint and carries a vertex when exactly one
endpoint is inside, at ``p_lo + t (p_hi - p_lo)``, ``t = clamp((level - v_lo) / (v_hi - v_lo), 0, 1)`` (a NaN quotient counts as 0);
vertices by owner point then axis, faces by cell then table order, vertex ids local to the scene.  The oracle takes the kernel's fp32
lattice values and computes everything else in fp64.

The SCAN LEDGER restates the tile sizes of csrc/lp_mesh.hip: a workgroup of the lattice passes holds ``MC_TILE`` points, a workgroup
of a scan level ``MC_SCAN`` entries, and the host adds a level whenever one does not fit a single workgroup.  ``scan_levels`` is the
number of scan launches; ``SCAN_THRESHOLDS`` are the point counts beyond which one more tile / level exists.  The host test asserts
that the GPU tests' lattices cross each of them.
"""
from __future__ import annotations

import importlib.util
import os
from typing import NamedTuple, Optional

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GENERATOR = os.path.join(REPO, "scripts", "gen_mc_table.py")
HEADER = os.path.join(REPO, "lightplane_amd", "csrc", "lp_mc_table.h")


def generator():
    spec = importlib.util.spec_from_file_location("gen_mc_table", GENERATOR)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = generator()
TABLE = np.array(GEN.build_table(), dtype=np.int64)                       # [256, 16]: triangles, 15 edges
EDGE_LO = np.array([a for a, _ in GEN.EDGES], dtype=np.int64)             # lower corner of every cube edge
EDGE_AXIS = np.array([(a ^ b).bit_length() - 1 for a, b in GEN.EDGES], dtype=np.int64)

# ---- the scan ledger (csrc/lp_mesh.hip: MC_TILE, MC_SCAN, mesh_layout) ----------------------------------------------------------------
MC_TILE = 256
MC_SCAN = 256
#: more than one tile; more than one workgroup of scan level 0 (a second level + one add launch); ... of level 1 (a third level)
SCAN_THRESHOLDS = (MC_TILE, MC_TILE * MC_SCAN, MC_TILE * MC_SCAN * MC_SCAN)


def scan_levels(n_points: int) -> int:
    """Scan launches of a lattice of ``n_points`` points (mesh_layout: levels until one fits a workgroup)."""
    cnt, levels = -(-n_points // MC_TILE), 1
    while cnt > MC_SCAN:
        cnt, levels = -(-cnt // MC_SCAN), levels + 1
    return levels


def workspace_bytes(n_points: int) -> int:
    """mesh_layout's total: the words (rounded up to 16 bytes), 16 bytes per entry of every scan level, 16 bytes for the total."""
    total = (n_points * 4 + 15) // 16 * 16
    cnt = -(-n_points // MC_TILE)
    while True:
        total += 16 * cnt
        if cnt <= MC_SCAN:
            return total + 16
        cnt = -(-cnt // MC_SCAN)


#: lattices of the random-volume GPU tests, [B, D, H, W]; the last one crosses every threshold below the top level of the hierarchy for
#: point counts below 2^31 (three scan launches, two add launches)
NOISE_SHAPES = ((2, 9, 7, 11), (1, 33, 31, 37))
MID_SHAPE = (1, 47, 41, 43)        # two scan levels
DEEP_SHAPE = (1, 259, 257, 253)    # three


# ---- the oracle -----------------------------------------------------------------------------------------------------------------------
class OracleMesh(NamedTuple):
    vertices: np.ndarray            # [V, 3] float64
    faces: np.ndarray               # [F, 3] int64, local to the scene
    normals: Optional[np.ndarray]   # [V, 3] float64
    vertex_offsets: np.ndarray      # [B + 1] int64
    face_offsets: np.ndarray        # [B + 1] int64


def _lin(n):
    return np.linspace(-1.0, 1.0, n) if n > 1 else np.zeros(1)


def _gradient(vol, b, z, y, x):
    """-> [n, 3] float64: d value / d (x, y, z) at the given points, central differences in scene coordinates, one-sided at the border."""
    _, D, H, W = vol.shape
    out = np.zeros((b.shape[0], 3))
    for k, (idx, n) in enumerate(((x, W), (y, H), (z, D))):
        if n < 2:
            continue
        lo, hi = np.maximum(idx - 1, 0), np.minimum(idx + 1, n - 1)
        c = _lin(n)
        sel_lo, sel_hi = [b, z, y, x], [b, z, y, x]
        sel_lo[3 - k], sel_hi[3 - k] = lo, hi
        out[:, k] = (vol[tuple(sel_hi)].astype(np.float64) - vol[tuple(sel_lo)].astype(np.float64)) / (c[hi] - c[lo])
    return out


def marching_cubes(volume: np.ndarray, level: float, with_normals: bool = False) -> OracleMesh:
    """The contract above on a float32 ``[B, D, H, W]`` array."""
    vol = np.ascontiguousarray(volume, dtype=np.float32)
    if vol.ndim == 3:
        vol = vol[None]
    B, D, H, W = vol.shape
    lvl32 = np.float32(level)
    with np.errstate(invalid="ignore"):
        inside = vol >= lvl32
    empty = OracleMesh(np.zeros((0, 3)), np.zeros((0, 3), np.int64), np.zeros((0, 3)) if with_normals else None,
                       np.zeros(B + 1, np.int64), np.zeros(B + 1, np.int64))
    if min(D, H, W) < 2:
        return empty
    # active owned edges, [B, D, H, W, 3] in axis order x, y, z
    act = np.zeros((B, D, H, W, 3), dtype=bool)
    act[:, :, :, :-1, 0] = inside[:, :, :, :-1] != inside[:, :, :, 1:]
    act[:, :, :-1, :, 1] = inside[:, :, :-1, :] != inside[:, :, 1:, :]
    act[:, :-1, :, :, 2] = inside[:, :-1, :, :] != inside[:, 1:, :, :]
    flat = act.reshape(-1)
    vid = np.cumsum(flat, dtype=np.int64) - 1                 # global vertex id of slot 3 n + axis (where active)
    slots = np.flatnonzero(flat)
    n_own, axis = slots // 3, slots % 3
    x, y, z, b = n_own % W, (n_own // W) % H, (n_own // (W * H)) % D, n_own // (W * H * D)
    step = np.stack([axis == 0, axis == 1, axis == 2], axis=1).astype(np.int64)
    x1, y1, z1 = x + step[:, 0], y + step[:, 1], z + step[:, 2]
    v0 = vol[b, z, y, x].astype(np.float64)
    v1 = vol[b, z1, y1, x1].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (np.float64(lvl32) - v0) / (v1 - v0)
    t = np.where(np.isnan(t), 0.0, np.clip(t, 0.0, 1.0))
    cx, cy, cz = _lin(W), _lin(H), _lin(D)
    p0 = np.stack([cx[x], cy[y], cz[z]], axis=1)
    p1 = np.stack([cx[x1], cy[y1], cz[z1]], axis=1)
    vertices = p0 + t[:, None] * (p1 - p0)
    scene = W * H * D
    bounds = np.arange(B + 1, dtype=np.int64) * scene
    vertex_offsets = np.searchsorted(n_own, bounds, side="left").astype(np.int64)
    normals = None
    if with_normals:
        with np.errstate(invalid="ignore", over="ignore"):
            g0, g1 = _gradient(vol, b, z, y, x), _gradient(vol, b, z1, y1, x1)
            g = g0 + t[:, None] * (g1 - g0)
            length = np.sqrt((g * g).sum(axis=1))
        ok = np.isfinite(length) & (length > 0)
        normals = np.where(ok[:, None], -g / np.where(ok, length, 1.0)[:, None], 0.0)
    # cells
    ins = inside.astype(np.uint8)
    case = np.zeros((B, D - 1, H - 1, W - 1), dtype=np.uint8)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        case |= ins[:, dz:D - 1 + dz, dy:H - 1 + dy, dx:W - 1 + dx] << c
    ntri_cell = TABLE[:, 0][case]
    cb, cz_, cy_, cx_ = np.nonzero(ntri_cell)                 # ascending in (b, z, y, x) = ascending in n
    n_cell = ((cb * D + cz_) * H + cy_) * W + cx_
    cases = case[cb, cz_, cy_, cx_].astype(np.int64)
    nt = TABLE[cases, 0]
    rep = np.repeat(np.arange(n_cell.shape[0]), nt)
    tri = np.arange(rep.shape[0]) - np.repeat(np.cumsum(nt) - nt, nt)       # index of the triangle inside its cell
    edges = TABLE[cases[rep][:, None], 1 + 3 * tri[:, None] + np.arange(3)[None, :]]   # [F, 3] cube edges
    lo = EDGE_LO[edges]
    owner = n_cell[rep][:, None] + (lo & 1) + ((lo >> 1) & 1) * W + ((lo >> 2) & 1) * W * H
    gid = vid[owner * 3 + EDGE_AXIS[edges]]
    assert flat[owner * 3 + EDGE_AXIS[edges]].all(), "a triangle uses an edge that is not crossed"
    face_scene = n_cell[rep] // scene
    faces = gid - vertex_offsets[face_scene][:, None]
    face_offsets = np.searchsorted(n_cell[rep], bounds, side="left").astype(np.int64)
    return OracleMesh(vertices, faces, normals, vertex_offsets, face_offsets)


# ---- properties of a mesh ---------------------------------------------------------------------------------------------------------------
def directed_edges(faces: np.ndarray, n_vertices: int) -> np.ndarray:
    """Codes a * V + b of the 3 F directed edges of the faces."""
    f = np.asarray(faces, dtype=np.int64)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    return a * max(n_vertices, 1) + b


def closed_and_oriented(faces: np.ndarray, n_vertices: int) -> bool:
    """Every directed edge occurs exactly once and its reverse exactly once (a closed, consistently oriented manifold mesh)."""
    f = np.asarray(faces, dtype=np.int64)
    if f.shape[0] == 0:
        return True
    if f.min() < 0 or f.max() >= n_vertices:
        return False
    fwd = np.sort(directed_edges(f, n_vertices))
    rev = np.sort(directed_edges(f[:, ::-1], n_vertices))
    return bool((np.diff(fwd) != 0).all() and np.array_equal(fwd, rev))


def signed_volume(vertices: np.ndarray, faces: np.ndarray) -> float:
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    return float((v[f[:, 0]] * np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def euler_characteristic(faces: np.ndarray, n_vertices: int) -> int:
    f = np.asarray(faces, dtype=np.int64)
    used = np.unique(f).shape[0]
    und = np.unique(np.sort(np.stack([directed_edges(f, n_vertices) // max(n_vertices, 1),
                                      directed_edges(f, n_vertices) % max(n_vertices, 1)], axis=1), axis=1), axis=0).shape[0]
    return used - und + f.shape[0]


def scenes(mesh):
    """(vertices, faces[, normals]) of every scene of an OracleMesh-like tuple of numpy arrays."""
    vo, fo = np.asarray(mesh.vertex_offsets), np.asarray(mesh.face_offsets)
    for b in range(vo.shape[0] - 1):
        yield mesh.vertices[vo[b]:vo[b + 1]], mesh.faces[fo[b]:fo[b + 1]]


# ---- lattices ----------------------------------------------------------------------------------------------------------------------------
def single_cell_cases() -> np.ndarray:
    """[256, 2, 2, 2]: scene c has corner i inside (+ magnitude) iff bit i of c; level 0."""
    rng = np.random.default_rng(11)
    c = np.arange(256)[:, None]
    sign = np.where((c >> np.arange(8)[None, :]) & 1, 1.0, -1.0)
    mag = 0.25 + 0.75 * rng.random((256, 8))
    return (sign * mag).reshape(256, 2, 2, 2).astype(np.float32)      # corner i = (x, y, z) bits = index [z, y, x]


def two_cell_cases(axis: int) -> np.ndarray:
    """[4096, ...]: every sign pattern of the 12 corners of two cells that share a face across ``axis`` (0 = x, 1 = y, 2 = z), inside a
    layer of outside values: [4096, 4, 4, 5] for x and its permutations for y and z; level 0."""
    rng = np.random.default_rng(12 + axis)
    p = np.arange(4096)[:, None]
    sign = np.where((p >> np.arange(12)[None, :]) & 1, 1.0, -1.0)
    mag = 0.25 + 0.75 * rng.random((4096, 12))
    core = (sign * mag).reshape(4096, 2, 2, 3)                        # [z, y, x] with x the long axis
    vol = -(0.25 + 0.75 * rng.random((4096, 4, 4, 5)))
    vol[:, 1:3, 1:3, 1:4] = core
    perm = {0: (0, 1, 2, 3), 1: (0, 1, 3, 2), 2: (0, 3, 2, 1)}[axis]    # the long axis becomes W, H or D
    return np.ascontiguousarray(vol.transpose(perm)).astype(np.float32)


def sphere(n: int, radius: float = 0.6, size=None) -> np.ndarray:
    """[1, D, H, W] lattice of radius - |p| (``size`` = (D, H, W), default n^3)."""
    D, H, W = size or (n, n, n)
    zz, yy, xx = np.meshgrid(_lin(D), _lin(H), _lin(W), indexing="ij")
    return (radius - np.sqrt(xx * xx + yy * yy + zz * zz))[None].astype(np.float32)


def sin_product(size, freq=(1.3, 1.7, 1.1), batch=1) -> np.ndarray:
    """A smooth field whose gradient stays away from zero near its zero set: sum of sines of the three coordinates plus a linear
    ramp along x (|grad| >= d/dx >= 1.5 - 0.3 * 1.3 > 1.1 everywhere)."""
    D, H, W = size
    zz, yy, xx = np.meshgrid(_lin(D), _lin(H), _lin(W), indexing="ij")
    out = []
    for b in range(batch):
        f = 1.5 * xx + 0.3 * (np.sin(freq[0] * xx + b) + np.sin(freq[1] * yy - b) + np.sin(freq[2] * zz + 0.5 * b))
        out.append(f)
    return np.stack(out).astype(np.float32)


def noise(shape, seed=0) -> np.ndarray:
    return np.random.default_rng(100 + seed).standard_normal(shape).astype(np.float32)


def padded_noise(shape, seed=0) -> np.ndarray:
    """Noise inside one layer of outside values: the level-0 surface is closed."""
    vol = noise(shape, seed)
    out = -np.abs(vol) - 0.1
    out[:, 1:-1, 1:-1, 1:-1] = vol[:, 1:-1, 1:-1, 1:-1]
    return out


def sparse_blobs(shape, seed=0) -> np.ndarray:
    """A mostly empty (-1) lattice with noise blocks next to its first, at a middle and next to its last cells: the prefix sums that reach the last
    block cross every tile and every level of the scan."""
    B, D, H, W = shape
    rng = np.random.default_rng(200 + seed)
    vol = np.full(shape, -1.0, dtype=np.float32)
    k = 6
    for z0, y0, x0 in ((1, 1, 1), (D // 2, H // 3, W // 2), (D - k - 1, H - k - 1, W - k - 1)):  # one layer inside: the surface is closed
        vol[:, z0:z0 + k, y0:y0 + k, x0:x0 + k] = rng.standard_normal((B, k, k, k)).astype(np.float32)
    return vol

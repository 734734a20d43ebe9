#!/usr/bin/env python
"""Generate the marching-cubes triangulation table of lightplane_amd/csrc/lp_mc_table.h.

    python scripts/gen_mc_table.py            # prints the header
    python scripts/gen_mc_table.py --write    # rewrites lightplane_amd/csrc/lp_mc_table.h

The table is constructed, not copied:
  * cube corner i sits at (x, y, z) = (i & 1, (i >> 1) & 1, (i >> 2) & 1); bit i of a case is set when corner i is inside
    (value >= level);
  * the 12 cube edges are the corner pairs that differ in one bit, numbered in lexicographic order of (lower, higher corner);
  * on each of the 6 faces the 4 corners are walked counter-clockwise as seen from outside the cube, and every maximal run of inside
    corners yields one directed contour segment from the crossed edge before the run to the crossed edge after it.  Two diagonal
    inside corners of a face are therefore always separated, and because the rule reads the four corner flags of the face only, the
    two cells that share a face draw the same segments on it (in opposite directions): the mesh is watertight by construction;
  * that direction makes the triangle normals point towards the lower values (-grad): the inside part of a face, walked
    counter-clockwise from outside, runs entry crossing -> inside corners -> exit crossing and closes along the segment exit -> entry,
    so the surface patch on the other side of the segment carries it as entry -> exit;
  * every crossed edge has one incoming and one outgoing segment; following them gives closed loops (started at the lowest unvisited
    crossed edge), and each loop is triangulated as a fan whose apex is the first rotation of the loop for which no fan diagonal
    joins two crossings that lie on one cube face -- such a diagonal can coincide with the neighbour cell's segment on that face and
    make an edge with four triangles.
Row c of the table: byte 0 = number of triangles (0 .. 5), bytes 1 .. 15 = their cube edges, three per triangle, 0 where unused.
"""
import os
import sys

CORNERS = [(i & 1, (i >> 1) & 1, (i >> 2) & 1) for i in range(8)]
EDGES = [(a, b) for a in range(8) for b in range(a + 1, 8) if bin(a ^ b).count("1") == 1]  # lexicographic by construction
EDGE_ID = {e: i for i, e in enumerate(EDGES)}
MAX_TRIANGLES = 5


def _cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def faces():
    """The 6 faces as 4 corners each, counter-clockwise as seen from outside the cube; order: axis x, y, z, low side first."""
    out = []
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3  # (e_u x e_v = e_axis)
        for side in (0, 1):
            loop = []
            for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1)):  # counter-clockwise around +e_axis
                c = [0, 0, 0]
                c[axis], c[u], c[v] = side, du, dv
                loop.append(c[0] | (c[1] << 1) | (c[2] << 2))
            if side == 0:  # the outward normal is -e_axis
                loop = [loop[0]] + loop[:0:-1]
            p = [CORNERS[c] for c in loop]
            n = _cross(tuple(p[1][k] - p[0][k] for k in range(3)), tuple(p[2][k] - p[1][k] for k in range(3)))
            assert n[axis] == (1 if side else -1) and n[u] == 0 and n[v] == 0
            out.append(tuple(loop))
    return out


FACES = faces()


def edge_of(a, b):
    return EDGE_ID[(min(a, b), max(a, b))]


def edges_share_face(e, f):
    """Both cube edges lie in one face of the cube."""
    pts = [CORNERS[c] for c in EDGES[e] + EDGES[f]]
    return any(all(p[axis] == side for p in pts) for axis in range(3) for side in (0, 1))


def segments(case):
    """Directed contour segments (from edge, to edge) of a case, face by face."""
    segs = []
    for loop in FACES:
        inside = [(case >> c) & 1 for c in loop]
        if sum(inside) in (0, 4):
            continue
        for s in range(4):
            if inside[s] and not inside[s - 1]:  # a run of inside corners starts at s
                e = s
                while inside[(e + 1) % 4]:
                    e += 1
                segs.append((edge_of(loop[s - 1], loop[s]), edge_of(loop[e % 4], loop[(e + 1) % 4])))
    return segs


def loops(case):
    """Closed loops of crossed edges of a case, each started at its lowest edge, in ascending order of that edge."""
    segs = segments(case)
    nxt = {}
    for a, b in segs:
        assert a not in nxt, "a crossed edge has one outgoing segment"
        nxt[a] = b
    assert sorted(nxt) == sorted(b for _, b in segs), "a crossed edge has one incoming segment"
    out, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start
        out.append(loop)
    return out


def fan(loop):
    """Triangles of a loop: the fan of the first rotation without a diagonal inside a cube face."""
    k = len(loop)
    for r in range(k):
        rot = loop[r:] + loop[:r]
        if not any(edges_share_face(rot[0], rot[i]) for i in range(2, k - 1)):
            return [(rot[0], rot[i], rot[i + 1]) for i in range(1, k - 1)]
    raise AssertionError(f"no admissible apex for loop {loop}")


def build_table():
    """256 rows of 16 ints: [n_triangles, 15 edge numbers]."""
    table = []
    for case in range(256):
        tris = [t for loop in loops(case) for t in fan(loop)]
        assert len(tris) <= MAX_TRIANGLES
        flat = [e for t in tris for e in t]
        table.append([len(tris)] + flat + [0] * (15 - len(flat)))
    return table


def emit(table=None):
    table = build_table() if table is None else table
    n_tri = sum(r[0] for r in table)
    lines = [
        "// lp_mc_table.h -- marching-cubes triangulation table.  GENERATED by scripts/gen_mc_table.py: do not edit, regenerate.",
        "// Corner i at (i & 1, (i >> 1) & 1, (i >> 2) & 1), bit i of the case = corner i inside; the 12 edges are the corner pairs that",
        "// differ in one bit in lexicographic order.  Row c: byte 0 = triangles of case c, bytes 1 .. 15 = their cube edges.",
        f"// 256 cases, {n_tri} triangles, at most {max(r[0] for r in table)} per case (DESIGN.md 4.15).",
        "#pragma once",
        "#define LP_MC_EDGE_LO {" + ", ".join(str(a) for a, _ in EDGES) + "}  /* lower corner of every edge */",
        "#define LP_MC_EDGE_AXIS {" + ", ".join(str((a ^ b).bit_length() - 1) for a, b in EDGES) + "}  /* 0 = x, 1 = y, 2 = z */",
        "#define LP_MC_TABLE_ROWS \\",
    ]
    for c, row in enumerate(table):
        lines.append("  {" + ", ".join(f"{v:2d}" for v in row) + "}" + (", \\" if c < 255 else ""))
    return "\n".join(lines) + "\n"


HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "lightplane_amd", "csrc", "lp_mc_table.h")

if __name__ == "__main__":
    text = emit()
    if "--write" in sys.argv:
        with open(HEADER, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)

"""Writes deep-video-mvs_amd/csrc/marching_cubes_tables.h: the 256-case marching-cubes tables of csrc/marching_cubes.hip.

The triangle table is derived, not typed in: for every case the surface's trace on each cube face is fixed by that face's four
corner signs alone (the segments cut off the INSIDE corners; on an ambiguous face, two diagonal inside corners are separated),
so two cubes that share a face cut it the same way and the mesh has no cracks.  The face segments are directed (outside
corners on the left, seen from outside the cube), chained into closed loops, and each loop is fanned from its first vertex:
every triangle is counter-clockwise seen from the outside (value >= level) side.

    python tools/gen_marching_cubes_tables.py            # rewrites the header
    python tools/gen_marching_cubes_tables.py --check    # exit 1 when the committed header differs
"""
import os
import sys

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
HEADER = os.path.join(ROOT, "deep-video-mvs_amd", "csrc", "marching_cubes_tables.h")

CORNERS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
EDGES = [(0, 1), (1, 2), (3, 2), (0, 3), (4, 5), (5, 6), (7, 6), (4, 7), (0, 4), (1, 5), (2, 6), (3, 7)]   # (low, high) corner


def edge_owner(e):
    """(di, dj, dk, axis): the edge is the +axis edge of the voxel at the cube's origin + (di, dj, dk)."""
    a, b = EDGES[e]
    lo, hi = np.array(CORNERS[a]), np.array(CORNERS[b])
    return tuple(int(v) for v in lo) + (int(np.argmax(hi - lo)),)


def faces_ccw():
    """The six faces as corner lists, counter-clockwise seen from outside the cube."""
    out = []
    for axis in range(3):
        for side in (0, 1):
            cs = [c for c in range(8) if CORNERS[c][axis] == side]
            n = np.zeros(3)
            n[axis] = 1.0 if side else -1.0
            centre = np.mean([CORNERS[c] for c in cs], axis=0)
            u = np.zeros(3)
            u[(axis + 1) % 3] = 1.0
            v = np.cross(n, u)
            cs.sort(key=lambda c: np.arctan2(np.dot(np.array(CORNERS[c]) - centre, v), np.dot(np.array(CORNERS[c]) - centre, u)))
            out.append(cs)
    return out


def edge_of(a, b):
    return next(e for e, ab in enumerate(EDGES) if set(ab) == {a, b})


def triangles(case):
    inside = [(case >> c) & 1 for c in range(8)]
    nxt = {}
    for q in faces_ccw():
        for k in range(4):
            # a run of inside corners starts at q[k]: the segment goes from the edge entering it to the edge leaving it
            if inside[q[k]] and not inside[q[k - 1]]:
                m = k
                while inside[q[(m + 1) % 4]]:
                    m += 1
                start, end = edge_of(q[k - 1], q[k]), edge_of(q[m % 4], q[(m + 1) % 4])
                assert start not in nxt
                nxt[start] = end
    tris = []
    while nxt:
        loop = [min(nxt)]
        while nxt[loop[-1]] != loop[0]:
            loop.append(nxt[loop[-1]])
        for e in loop:
            del nxt[e]
        tris += triangulate(loop)
    return tris


def share_face(e1, e2):
    return any(set(EDGES[e1]) <= set(q) and set(EDGES[e2]) <= set(q) for q in faces_ccw())


def triangulate(loop):
    """Triangles of a loop, in loop order (so counter-clockwise like the loop), whose diagonals never join two vertices that lie
    on one cube face: the cube across that face could draw the same diagonal, and the edge would then carry four triangles.
    A fan from the earliest vertex that allows one; otherwise the first valid triangulation in a fixed search order."""
    n = len(loop)

    def ok(a, b):   # positions a < b in the polygon being split
        return b - a == 1 or (a == 0 and b == n - 1) or not share_face(loop[a], loop[b])

    for s in range(n):
        idx = [(s + i) % n for i in range(n)]
        if all(ok(min(idx[0], idx[i]), max(idx[0], idx[i])) for i in range(2, n - 1)):
            return [(loop[idx[0]], loop[idx[i]], loop[idx[i + 1]]) for i in range(1, n - 1)]

    def split(ids):  # ids: increasing positions of a sub-polygon; returns triangles or None
        if len(ids) < 3:
            return []
        a, b = ids[0], ids[-1]
        for m in range(1, len(ids) - 1):
            c = ids[m]
            if ok(a, c) and ok(c, b):
                left, right = split(ids[:m + 1]), split(ids[m:])
                if left is not None and right is not None:
                    return left + [(loop[a], loop[c], loop[b])] + right
        return None

    tris = split(list(range(n)))
    assert tris is not None, f"no crack-free triangulation of the loop {loop}"
    return tris


def render():
    cases = [triangles(c) for c in range(256)]
    max_tris = max(len(t) for t in cases)
    width = 3 * max_tris + 1
    edge_mask = []
    for c in range(256):
        m = 0
        for e, (a, b) in enumerate(EDGES):
            if ((c >> a) & 1) != ((c >> b) & 1):
                m |= 1 << e
        edge_mask.append(m)
    lines = [
        "// Marching-cubes case tables of csrc/marching_cubes.hip -- the only copy: tests/marching_cubes_cpu.py parses this file.",
        "// Generated by tools/gen_marching_cubes_tables.py; do not edit by hand.",
        "//",
        "// Corner c of the cube whose lowest corner is voxel (i, j, k) sits at (i, j, k) + offset:",
    ]
    lines += [f"//   corner {c}: (+{d[0]}, +{d[1]}, +{d[2]})" for c, d in enumerate(CORNERS)]
    lines += ["// Edge e joins corners kMcEdgeCorners[e] (low, high) and is the +axis edge of the voxel at (i, j, k) + (di, dj, dk):"]
    for e in range(12):
        di, dj, dk, ax = edge_owner(e)
        lines.append(f"//   edge {e:2d}: corners {EDGES[e][0]}-{EDGES[e][1]}, owner (+{di}, +{dj}, +{dk}), axis {'xyz'[ax]}")
    lines += [
        "// Case index: bit c set <=> corner c is inside (value < level).  kMcTriTable[case] lists triangles as edge triples,",
        "// terminated by -1; each is counter-clockwise seen from the outside (value >= level) side.  A face's cut depends only on",
        "// its four corners (inside corners are cut off one by one; on an ambiguous face the two inside corners are separated),",
        "// so neighbouring cubes agree and the surface is closed.",
        "#pragma once",
        "",
        f"#define DVMVS_MC_MAX_TRIS {max_tris}",
        "",
        "static constexpr unsigned char kMcEdgeCorners[12][2] = {" + ", ".join("{%d, %d}" % ab for ab in EDGES) + "};",
        "static constexpr unsigned char kMcEdgeOwner[12][4] = {" + ", ".join("{%d, %d, %d, %d}" % edge_owner(e) for e in range(12)) + "};",
        "",
        "static constexpr unsigned short kMcEdgeTable[256] = {",
    ]
    for r in range(0, 256, 16):
        lines.append("    " + ", ".join("0x%03x" % m for m in edge_mask[r:r + 16]) + ",")
    lines += ["};", "", "static constexpr unsigned char kMcTriCount[256] = {"]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(len(t)) for t in cases[r:r + 32]) + ",")
    lines += ["};", "", f"static constexpr signed char kMcTriTable[256][{width}] = {{"]
    for c, t in enumerate(cases):
        row = [e for tri in t for e in tri] + [-1] * (width - 3 * len(t))
        lines.append("    {" + ", ".join(str(v) for v in row) + "},")
    lines += ["};", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    text = render()
    if "--check" in sys.argv:
        sys.exit(0 if open(HEADER).read() == text else 1)
    with open(HEADER, "w") as f:
        f.write(text)
    print(f"wrote {HEADER}")

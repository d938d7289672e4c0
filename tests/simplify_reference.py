"""Meshes for the mesh-simplification tests (tests/test_simplify_reference.py on the host, tests/test_simplify_gpu.py on the GPU): each
builder returns a dict ``verts`` float32 [V,3], ``faces`` int32 [F,3], ``normals`` float32 [V,3], ``colors`` uint8 [V,3] and ``voxel``, the
cell the case is simplified with.  The builders are deterministic; ``host(name, contraction)`` computes the host definition of a case once
and hands the same, read-only arrays to every test."""
import functools

import numpy as np

from dvmvs.simplify import CONTRACTIONS, simplify_mesh

CUBE_OFFSET = np.array([0.013, 0.027, 0.041])
CUBE_CELL = 0.3
FAR_SHIFT = np.array([500.0, -300.0, 40.0])


def _mesh(verts, faces, voxel, seed=0):
    rng = np.random.default_rng(2000 + seed)
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    normals = rng.standard_normal(verts.shape).astype(np.float32)
    colors = rng.integers(0, 256, verts.shape, dtype=np.uint8)
    return {"verts": verts, "faces": faces, "normals": normals, "colors": colors, "voxel": voxel}


def _grid_faces(nu, nv, first=0):
    """The 2 nu nv triangles of a grid of (nu + 1) x (nv + 1) vertices numbered row by row from ``first``."""
    u, v = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    a = first + (u * (nv + 1) + v).reshape(-1)
    b, c, d = a + nv + 1, a + nv + 2, a + 1
    return np.concatenate([np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)])


def cube_mesh(n=12):
    """The surface of the unit cube [0, 1]^3, each side ``n`` x ``n`` quads with its own vertices (the sides are not welded; clustering
    welds them), float64 vertices and the faces."""
    t = np.linspace(0.0, 1.0, n + 1)
    u, v = (g.reshape(-1) for g in np.meshgrid(t, t, indexing="ij"))
    verts, faces = [], []
    for axis in range(3):
        for side in (0.0, 1.0):
            p = np.empty((len(u), 3))
            p[:, axis], p[:, (axis + 1) % 3], p[:, (axis + 2) % 3] = side, u, v
            quads = _grid_faces(n, n, first=sum(len(x) for x in verts))
            faces.append(quads if side else quads[:, ::-1])          # outward on both sides
            verts.append(p)
    return np.concatenate(verts), np.concatenate(faces)


def cube():
    """The unit cube, 12 x 12 quads a side, offset by (0.013, 0.027, 0.041), at cell 0.3: 56 clusters, of rank 1 / 2 / 3 = 24 / 24 / 8."""
    verts, faces = cube_mesh()
    return _mesh(verts + CUBE_OFFSET, faces, CUBE_CELL, 1)


def far():
    """The cube translated by (500, -300, 40): the sums about each cluster's own mean must find the same ranks."""
    verts, faces = cube_mesh()
    return _mesh(verts + CUBE_OFFSET + FAR_SHIFT, faces, CUBE_CELL, 2)


PLANE_NORMAL = np.array([0.3, -0.5, 0.81]) / np.linalg.norm([0.3, -0.5, 0.81])
PLANE_POINT = np.array([0.2, 0.1, -0.3])


def plane():
    """One flat 40 x 30 grid of 2.5 cm quads in a plane tilted off every axis, at cell 0.11: rank 1 everywhere."""
    e1 = np.cross(PLANE_NORMAL, [1.0, 0.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(PLANE_NORMAL, e1)
    u, v = (g.reshape(-1) for g in np.meshgrid(np.arange(41) * 0.025, np.arange(31) * 0.025, indexing="ij"))
    verts = PLANE_POINT + u[:, None] * e1 + v[:, None] * e2
    return _mesh(verts, _grid_faces(40, 30), 0.11, 3)


def single_cell():
    """One triangle whose corners share a cell: nothing survives."""
    return _mesh([[0.0, 0.0, 0.0], [0.01, 0.0, 0.0], [0.0, 0.01, 0.0]], [[0, 1, 2]], 0.5, 4)


def duplicates():
    """Five vertices a metre apart at cell 0.5 (one cluster each; ascending keys are vertices 0, 3, 2, 1, 4 -> clusters 0, 3, 2, 1, 4).
    Faces: (0,1,2) three times under its three rotations (the first stays), its opposite orientation (0,2,1) twice (the first stays),
    a face with the index -1, one with the index V, a face that uses a vertex twice, and (1,2,4)."""
    verts = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]]
    faces = [[0, 1, 2], [1, 2, 0], [0, 2, 1], [2, 0, 1], [-1, 1, 2], [0, 5, 2], [2, 1, 0], [3, 3, 4], [1, 2, 4]]
    return _mesh(verts, faces, 0.5, 5)


def long_run(n=3000):
    """A fan of ``n`` thin triangles whose hub and rim (radius 4 cm) fall into one 10 cm cell, every face with its three corners there,
    next to an ordinary 6 x 6 grid of 10 cm quads whose cells hold one vertex each: one cluster with 3 n incidences among small ones."""
    angle = np.arange(n + 1) * (1.5 * np.pi / n)
    rim = np.stack([0.05 + 0.04 * np.cos(angle), 0.05 + 0.04 * np.sin(angle), 0.05 + 0.01 * np.sin(3 * angle)], axis=1)
    hub = np.array([[0.05, 0.05, 0.06]])
    k = np.arange(n)
    fan = np.stack([np.zeros(n, dtype=np.int64), 1 + k, 2 + k], axis=1)
    u, v = (g.reshape(-1) for g in np.meshgrid(np.arange(7) * 0.1, np.arange(7) * 0.1, indexing="ij"))
    grid = np.stack([0.15 + u, 0.05 + v, 0.05 + 0.02 * u], axis=1)
    link = np.array([[0, 1, n + 2], [0, n + 2, n + 3]])              # the fan's cell is joined to the grid: it keeps faces
    verts = np.concatenate([hub, rim, grid])
    return _mesh(verts, np.concatenate([fan, link, _grid_faces(6, 6, first=n + 2)]), 0.1, 6)


def sized(n_clusters):
    """``n_clusters`` cells in a row, each with two vertices a millimetre apart, a triangle strip over consecutive cells, the same
    strip through the cells' second vertices (duplicates), two faces with two corners in one cell (dropped) and the opposite orientations
    of the first two faces (kept): ``n_clusters`` clusters and ``n_clusters`` surviving faces out of ``2 n_clusters``, around the 1024
    that one scan block takes."""
    x = np.arange(n_clusters) * 0.1 + 0.05
    zig = np.where(np.arange(n_clusters) % 2 == 0, 0.0, 0.08)
    first = np.stack([x, 0.01 + zig, np.full(n_clusters, 0.02)], axis=1)
    second = first + [0.001, 0.001, 0.0]
    verts = np.concatenate([first, second, [[0.0, 0.01, 0.02]]])     # the last, which no face uses, puts the others in mid-cell
    k = np.arange(n_clusters - 2)
    strip = np.stack([k, k + 1, k + 2], axis=1)
    strip[1::2] = strip[1::2][:, [0, 2, 1]]
    twin = np.stack([k + n_clusters, k + 1, k + 2], axis=1)          # the same cells through the second vertices: duplicates
    twin[1::2] = twin[1::2][:, [0, 2, 1]]
    inner = np.stack([np.arange(2), np.arange(2) + n_clusters, np.arange(2) + 1], axis=1)      # two corners in one cell: dropped
    opposite = strip[:2][:, [0, 2, 1]]
    return _mesh(verts, np.concatenate([strip, twin, inner, opposite]), 0.1, 7)


def attributes():
    """Two cells joined to a third by faces.  In the first the members' normals cancel to zero and the colours' means sit on .5 (127.5,
    0.5, 254.5: halves go to even); in the second a normal is not finite."""
    verts = [[0.01, 0.01, 0.0], [0.02, 0.01, 0.0], [0.51, 0.0, 0.0], [0.52, 0.0, 0.0], [0.0, 0.51, 0.0], [0.01, 0.52, 0.3]]
    faces = [[0, 2, 4], [1, 3, 5], [0, 3, 4]]
    case = _mesh(verts, faces, 0.5, 8)
    case["normals"][:2] = [[0.25, -1.0, 0.5], [-0.25, 1.0, -0.5]]
    case["normals"][2:4] = [[0.0, 0.0, 1.0], [np.inf, 0.0, 0.0]]
    case["colors"][:2] = [[127, 0, 254], [128, 1, 255]]
    return case


def empty_both():
    return _mesh(np.zeros((0, 3)), np.zeros((0, 3)), 0.1, 9)


def empty_faces():
    return _mesh(np.random.default_rng(11).random((70, 3)), np.zeros((0, 3)), 0.2, 10)


def non_finite():
    """The duplicates with a coordinate at NaN: ``ValueError``."""
    case = duplicates()
    case["verts"][3, 1] = np.nan
    return case


def too_many_cells():
    """Two vertices 2^21 cells apart: ``ValueError``."""
    return _mesh([[0.0, 0.0, 0.0], [0.0, 2.0 ** 21 * 0.001, 0.0], [0.0, 0.0, 1.0]], [[0, 1, 2]], 0.001, 12)


CASES = {"empty_both": empty_both, "empty_faces": empty_faces, "single_cell": single_cell, "cube": cube, "plane": plane,
         "duplicates": duplicates, "long_run": long_run, "sized_1024": functools.partial(sized, 1024),
         "sized_1025": functools.partial(sized, 1025), "attributes": attributes, "far": far}
ERROR_CASES = {"non_finite": non_finite, "too_many_cells": too_many_cells}


@functools.lru_cache(maxsize=None)
def case(name):
    built = (CASES.get(name) or ERROR_CASES[name])()
    for a in built.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return built


@functools.lru_cache(maxsize=None)
def host(name, contraction="quadric", attributes=True):
    """``simplify_mesh(..., return_index=True)`` of a case, flattened to (verts, faces, normals, colors, vertex_cluster, face_index),
    computed once; the arrays are read-only."""
    assert contraction in CONTRACTIONS
    c = case(name)
    out = simplify_mesh(c["verts"], c["faces"], c["voxel"], c["normals"] if attributes else None, c["colors"] if attributes else None,
                        contraction, return_index=True)
    flat = out[:4] + out[4]
    for a in flat:
        if a is not None:
            a.setflags(write=False)
    return flat


def cube_distances(points, shift=CUBE_OFFSET):
    """``(the greatest distance of a point from the surface of the cube, the greatest distance of a true corner from its nearest
    point)`` of float32 points, in float64."""
    p = points.astype(np.float64) - shift
    outside = np.linalg.norm(np.maximum(np.maximum(-p, p - 1.0), 0.0), axis=1)
    inside = np.minimum(np.minimum(p, 1.0 - p).min(axis=1), np.inf)
    surface = np.where(outside > 0.0, outside, np.maximum(inside, 0.0))
    corners = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)])
    nearest = np.linalg.norm(corners[:, None, :] - p[None, :, :], axis=2).min(axis=1)
    return float(surface.max()), float(nearest.max())

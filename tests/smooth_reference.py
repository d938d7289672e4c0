"""Meshes and settings for the mesh-smoothing tests (tests/test_smooth_reference.py on the host, tests/test_smooth_gpu.py on the GPU): each
builder returns a dict ``verts`` float32 [V,3], ``faces`` int32 [F,3], ``normals`` float32 [V,3] and ``colors`` uint8 [V,3].  The builders
are deterministic; ``host(name, setting)`` computes the host definition of a case once and hands the same, read-only arrays to every
test."""
import functools

import numpy as np

from dvmvs.smooth import SmoothSettings, smooth_mesh, vertex_normals, vertex_rows

FAR_SHIFT = np.array([1000.0, -2000.0, 500.0])
PATCH_SHAPE = (9, 7)
PATCH_SPACING = 0.25

# every way a case is run: Laplacian at 1 and 3 iterations, Taubin at 2, both boundaries, no iteration, normals kept
SETTINGS = {
    "laplacian_1_free": SmoothSettings(1, "laplacian"),
    "laplacian_1_fixed": SmoothSettings(1, "laplacian", boundary="fixed"),
    "laplacian_3_free": SmoothSettings(3, "laplacian", lam=0.625),
    "laplacian_3_fixed": SmoothSettings(3, "laplacian", lam=1.0, boundary="fixed"),
    "taubin_2_free": SmoothSettings(2),
    "taubin_2_fixed": SmoothSettings(2, "taubin", 0.33, -0.34, "fixed"),
    "taubin_2_keep_normals": SmoothSettings(2, recompute_normals=False),
    "none": SmoothSettings(0),
    "none_keep_normals": SmoothSettings(0, "laplacian", recompute_normals=False),
}


def _mesh(verts, faces, seed=0, normals=None):
    rng = np.random.default_rng(3000 + seed)
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    if normals is None:
        normals = rng.standard_normal(verts.shape)
    colors = rng.integers(0, 256, verts.shape, dtype=np.uint8)
    return {"verts": verts, "faces": faces, "normals": np.ascontiguousarray(normals, dtype=np.float32), "colors": colors}


def _outward(verts, faces, centre):
    """``faces`` with every triangle wound counter-clockwise seen from outside ``centre``."""
    p = np.asarray(verts, dtype=np.float64)
    faces = np.array(faces, dtype=np.int64)
    n = np.cross(p[faces[:, 1]] - p[faces[:, 0]], p[faces[:, 2]] - p[faces[:, 0]])
    flip = np.einsum("ij,ij->i", n, p[faces].mean(axis=1) - centre) < 0
    faces[flip] = faces[flip][:, ::-1]
    return faces


def empty_both():
    return _mesh(np.zeros((0, 3)), np.zeros((0, 3)), 1)


def empty_faces():
    return _mesh(np.random.default_rng(1).standard_normal((5, 3)), np.zeros((0, 3)), 2)


def triangle():
    return _mesh([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.2, 0.9, 0.3]], [[0, 1, 2]], 3)


def tetrahedron():
    verts = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.1], [0.3, 0.9, 0.0], [0.4, 0.3, 0.8]])
    return _mesh(verts, _outward(verts, [[0, 1, 2], [0, 1, 3], [1, 2, 3], [0, 2, 3]], verts.mean(axis=0)), 4)


def _cube(shift):
    verts = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)])
    quads = [[0, 1, 3, 2], [4, 5, 7, 6], [0, 1, 5, 4], [2, 3, 7, 6], [0, 2, 6, 4], [1, 3, 7, 5]]
    faces = _outward(verts, [t for q in quads for t in ([q[0], q[1], q[2]], [q[0], q[2], q[3]])], np.full(3, 0.5))
    outward = (verts - 0.5) / np.linalg.norm(verts - 0.5, axis=1, keepdims=True)
    return verts + shift, faces, outward


def cube():
    """The unit cube: 8 vertices, 12 faces, colours and outward normals."""
    verts, faces, outward = _cube(np.zeros(3))
    return _mesh(verts, faces, 5, outward)


def far():
    """``cube`` translated by (1000, -2000, 500): float64 sums where float32 would cancel."""
    verts, faces, outward = _cube(FAR_SHIFT)
    return _mesh(verts, faces, 5, outward)


def icosphere(subdivisions):
    """The unit icosphere: float64 vertices and outward faces."""
    t = (1.0 + np.sqrt(5.0)) / 2.0
    verts = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1], [-t, 0, -1],
             [-t, 0, 1]]
    faces = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8], [3, 9, 4],
             [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    verts = [np.array(v, dtype=np.float64) / np.linalg.norm(v) for v in verts]
    for _ in range(subdivisions):
        middle, finer = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in middle:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                middle[key] = len(verts) - 1
            return middle[key]

        for a, b, c in faces:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            finer += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        faces = finer
    verts = np.array(verts)
    return verts, _outward(verts, faces, np.zeros(3))


def sphere_noisy():
    """The icosphere subdivided twice (162 vertices, 320 faces), every radius times 1 + 0.02 of a standard normal."""
    verts, faces = icosphere(2)
    assert verts.shape == (162, 3) and faces.shape == (320, 3)
    return _mesh(verts * (1.0 + 0.02 * np.random.default_rng(0).standard_normal(len(verts)))[:, None], faces, 6)


def shuffled():
    """``sphere_noisy`` with its vertices renumbered by a permutation: neighbours far apart in memory, rows that a face order does not sort."""
    c = sphere_noisy()
    new_of_old = np.random.default_rng(7).permutation(len(c["verts"]))
    out = {k: np.empty_like(c[k]) for k in ("verts", "normals", "colors")}
    for k in out:
        out[k][new_of_old] = c[k]
    out["faces"] = new_of_old[c["faces"]].astype(np.int32)
    return out


def patch():
    """A flat 9 x 7 grid at spacing 0.25 in z = 0, two triangles per square with the same diagonal everywhere."""
    nu, nv = PATCH_SHAPE
    u, v = (g.reshape(-1) for g in np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij"))
    verts = np.stack([u * PATCH_SPACING, v * PATCH_SPACING, np.zeros(len(u))], axis=1)
    a = (u * nv + v)[(u < nu - 1) & (v < nv - 1)]
    b, c, d = a + nv, a + nv + 1, a + 1
    return _mesh(verts, np.concatenate([np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)]), 8)


def fan():
    """A hub above a rim of 300 vertices, closed: the hub's row is far longer than a wave."""
    n = 300
    angle = 2.0 * np.pi * np.arange(n) / n
    rim = np.stack([np.cos(angle), np.sin(angle), 0.05 * np.sin(7.0 * angle)], axis=1)
    verts = np.concatenate([[[0.03, -0.02, 0.4]], rim])
    i = np.arange(n)
    return _mesh(verts, np.stack([np.zeros(n, dtype=np.int64), 1 + i, 1 + (i + 1) % n], axis=1), 9)


JUNK_VERTICES = 8
JUNK_FACES = [[0, 1, 2], [0, 1, 2], [2, 1, 0],      # a face three times, once the other way round: its pairs are emitted three times
              [1, 1, 3],                            # (a, a, b) does not count
              [-1, 2, 3], [2, 3, 8],                # an index of -1, an index of V
              [1, 2, 3], [1, 2, 4],                 # the edge (1, 2) now has more than three faces; (1, 3), (2, 3), (2, 4), (1, 4) have one
              [3, 4, 5], [5, 4, 3]]                 # an edge of two faces of opposite orientation is no boundary: vertex 5 is inside
# vertices 6 and 7 are used by no face
JUNK_ROWS = ([0, 2, 6, 10, 14, 18, 20, 20, 20],
             [1, 2, 0, 2, 3, 4, 0, 1, 3, 4, 1, 2, 4, 5, 1, 2, 3, 5, 3, 4],
             [False, True, True, True, True, False, False, False])


def junk():
    return _mesh(np.random.default_rng(11).standard_normal((JUNK_VERTICES, 3)), JUNK_FACES, 10)


def strip_1025():
    """A triangle strip of 1025 vertices: rows and offsets across workgroups, waves and the 1024-key chunks of the scans."""
    i = np.arange(1025)
    verts = np.stack([(i // 2) * 0.1, (i % 2) * 0.1, 0.02 * np.sin(0.37 * i)], axis=1)
    f = np.arange(1023)
    faces = np.stack([f, f + 1, f + 2], axis=1)
    faces[1::2] = faces[1::2][:, ::-1]
    return _mesh(verts, faces, 12)


CASES = {"empty_both": empty_both, "empty_faces": empty_faces, "triangle": triangle, "tetrahedron": tetrahedron, "cube": cube,
         "sphere_noisy": sphere_noisy, "patch": patch, "fan": fan, "junk": junk, "strip_1025": strip_1025, "shuffled": shuffled, "far": far}


def _freeze(arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def case(name):
    built = CASES[name]()
    _freeze(built.values())
    return built


@functools.lru_cache(maxsize=None)
def host(name, setting, attributes=True):
    """``smooth_mesh`` of a case with ``SETTINGS[setting]``: (verts, faces, normals, colors), computed once; the arrays are read-only."""
    c = case(name)
    out = smooth_mesh(c["verts"], c["faces"], SETTINGS[setting], c["normals"] if attributes else None, c["colors"] if attributes else None)
    _freeze(out)
    return out


@functools.lru_cache(maxsize=None)
def host_rows(name):
    c = case(name)
    out = vertex_rows(c["faces"], len(c["verts"]))
    _freeze(out)
    return out


@functools.lru_cache(maxsize=None)
def host_normals(name, fallback=False):
    c = case(name)
    out = vertex_normals(c["verts"], c["faces"], c["normals"] if fallback else None)
    out.setflags(write=False)
    return out


def radii(verts):
    """``(mean, standard deviation)`` of the distances of float32 points from the origin, in float64."""
    r = np.linalg.norm(np.asarray(verts).astype(np.float64), axis=1)
    return r.mean(), r.std()

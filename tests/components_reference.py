"""Meshes for the connected-component tests (tests/test_components_reference.py on the host, tests/test_components_gpu.py on the GPU): each
builder returns a dict ``verts`` float32 [V,3], ``faces`` int32 [F,3], ``normals`` float32 [V,3], ``colors`` uint8 [V,3].  The builders are
deterministic; ``host(case)`` computes the host definition of a case once and hands the same, read-only arrays to every test."""
import functools

import numpy as np

from dvmvs.components import ComponentFilter, filter_components, mesh_components

AREA_UNIT = 2.0 ** -32                     # square metres per unit of quantised area


def _mesh(verts, faces, seed=0):
    rng = np.random.default_rng(1000 + seed)
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    normals = rng.standard_normal(verts.shape).astype(np.float32)
    colors = rng.integers(0, 256, verts.shape, dtype=np.uint8)
    return {"verts": verts, "faces": faces, "normals": normals, "colors": colors}


TET = np.array([[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]])


def tetrahedra():
    """Two tetrahedra (vertices 0..3 with legs of 1 m, 4..7 with legs of 0.5 m), vertex 8 that no face uses, one face with the index V
    and one with -1.  labels 0 0 0 0 4 4 4 4 8; face labels 0 0 0 0 4 4 4 4 -1 -1; 4 faces each; areas 1.5 + sqrt(3)/2 and a quarter."""
    corner = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float64)
    verts = np.concatenate([corner, 0.5 * corner + [3.0, 0.0, 0.0], [[9.0, 9.0, 9.0]]])
    faces = np.concatenate([TET, TET + 4, [[0, 1, 9]], [[4, -1, 5]]])
    return _mesh(verts, faces, 1)


def strip(n_faces=20000, seed=5):
    """A triangle strip of ``n_faces`` faces whose vertices are numbered by a seeded permutation: one component whose union-find chains are
    deep, since neighbouring faces hook far-apart indices."""
    n = n_faces + 2
    i = np.arange(n)
    verts = np.stack([(i // 2) * 0.01, (i % 2) * 0.01, np.zeros(n)], axis=1)
    f = np.arange(n_faces)
    faces = np.stack([f, f + 1, f + 2], axis=1)
    perm = np.random.default_rng(seed).permutation(n)
    moved = np.empty_like(verts)
    moved[perm] = verts
    return _mesh(moved, perm[faces], 2)


def soup(n_verts=3000, n_faces=2500, seed=7):
    """Faces with uniform random indices: one giant component, many tiny ones, many vertices that no face uses."""
    rng = np.random.default_rng(seed)
    return _mesh(rng.random((n_verts, 3)), rng.integers(0, n_verts, (n_faces, 3)), 3)


def ties():
    """Components with equal areas and equal counts, for the tie rules of ``keep_largest``.  In the plane z = 0, in the order of their labels:
      label 0: ONE triangle of area 1 (legs 2 and 1);
      label 3: two triangles of area 1/2 each (a unit square): area 1, 2 faces;
      label 7: the same square moved: area 1, 2 faces;
      label 11, 14: single triangles of area 1/2.
    The greatest area, 1, is shared by labels 0, 3 and 7; the greater face count leaves 3 and 7; the smaller label is 3.  All coordinates are
    small integers, so the quantised areas are exactly 2^32 and 2^31 units."""
    def square(x):
        return [[x, 0, 0], [x + 1, 0, 0], [x + 1, 1, 0], [x, 1, 0]]
    verts = [[0, 0, 0], [2, 0, 0], [0, 1, 0]] + square(4) + square(8) + [[12, 0, 0], [13, 0, 0], [12, 1, 0]] + [[16, 0, 0], [17, 0, 0], [16, 1, 0]]
    faces = [[0, 1, 2], [3, 4, 5], [3, 5, 6], [7, 8, 9], [7, 9, 10], [11, 12, 13], [14, 15, 16]]
    return _mesh(verts, faces, 4)


SCAN_FACES = (0, 1, 1023, 1024, 1025, 3 * 1024 + 1)
SCAN_VERTS = (0, 1, 63, 64, 65, 1025)


def sized(n_faces, n_verts):
    """``n_faces`` faces with uniform random indices over ``n_verts`` vertices (all invalid when there is no vertex): the sizes around the
    boundaries of the scans (a workgroup takes 1024 elements, a wave 64)."""
    rng = np.random.default_rng(n_faces * 2053 + n_verts)
    faces = rng.integers(0, max(n_verts, 1), (n_faces, 3))
    return _mesh(rng.random((n_verts, 3)), faces, 5)


def nan_face():
    """The tetrahedra with a vertex of the second one at NaN: its faces have no finite area."""
    case = tetrahedra()
    case["verts"][5, 1] = np.nan
    return case


CASES = {"tetrahedra": tetrahedra, "strip": strip, "soup": soup, "ties": ties}
CASES.update({f"sized_{f}_{v}": functools.partial(sized, f, v) for f in SCAN_FACES for v in SCAN_VERTS})


@functools.lru_cache(maxsize=None)
def case(name):
    built = CASES[name]()
    for a in built.values():
        a.setflags(write=False)
    return built


@functools.lru_cache(maxsize=None)
def host(name):
    """``mesh_components`` of a case (with its areas), computed once; the arrays are read-only."""
    c = case(name)
    parts = mesh_components(c["faces"], len(c["verts"]), c["verts"])
    for a in parts.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return parts


def filters(name):
    """The filters a case is cleaned with: area only, faces only, both, largest, and largest failing a threshold.  The area threshold is
    the median area of the case's components (so that it separates them), the face threshold 2."""
    parts = host(name)
    areas = parts["area"][parts["face_count"] > 0]
    median = float(np.median(areas)) * AREA_UNIT if len(areas) else 0.25
    most = int(parts["face_count"].max()) if len(parts["face_count"]) else 0
    return (ComponentFilter(min_area=median), ComponentFilter(min_faces=2), ComponentFilter(min_area=median, min_faces=3),
            ComponentFilter(keep_largest=True), ComponentFilter(min_faces=most + 1, keep_largest=True), ComponentFilter())


@functools.lru_cache(maxsize=None)
def host_filtered(name, filter):
    c = case(name)
    out = filter_components(c["verts"], c["faces"], filter, c["normals"], c["colors"], return_index=True)
    return out[:4] + out[4]                # verts, faces, normals, colors, vertex_index, face_index


def scipy_labels(faces, n_verts):
    """The smallest-index labels from ``scipy.sparse.csgraph.connected_components`` over the edges of the valid faces."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    good = faces[np.all((faces >= 0) & (faces < n_verts), axis=1)]
    rows = np.concatenate([good[:, 0], good[:, 1], good[:, 2]])
    cols = np.concatenate([good[:, 1], good[:, 2], good[:, 0]])
    graph = coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(n_verts, n_verts)).tocsr()
    n, found = connected_components(graph, directed=False)
    smallest = np.full(n, n_verts, dtype=np.int64)
    np.minimum.at(smallest, found, np.arange(n_verts))
    return smallest[found].astype(np.int32)

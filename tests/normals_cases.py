"""The clouds that tests/test_normals_reference.py (CPU: vectorised host form against the scalar loop) and tests/test_normals_gpu.py (device
against host form) both run: numpy only, every case seeded.  Two kinds:
  SEARCH cases  ``(points, neighbours, max_distance, viewpoints, view)``: normals of a cloud against itself, the rows found by a search;
  ROW cases     ``(points, target, index, viewpoints, view)``: hand-made rows, separate clouds."""
import numpy as np


def sphere(n=1000, noise=0.01, seed=0, centre=(0.0, 0.0, 0.0)):
    """``(points float32 [n,3], directions float64 [n,3])``: a unit sphere with relative radial noise."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (d * (1.0 + noise * rng.normal(size=(n, 1))) + np.asarray(centre)).astype(np.float32), d


def far_plane(n=1000, seed=1, thickness=0.002):
    """A tilted noisy plane patch of 1 m, 100 m from the origin."""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(-0.5, 0.5, size=(2, n))
    normal = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    a = np.cross(normal, [1.0, 0.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(normal, a)
    points = np.array([60.0, -70.0, 40.0]) + u[:, None] * a + v[:, None] * b + thickness * rng.normal(size=(n, 1)) * normal
    return points.astype(np.float32), normal


def planar_lattice(n=8):
    g = np.arange(n, dtype=np.float32)
    x, y = np.meshgrid(g, g, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), np.full(n * n, 2.0, np.float32)], axis=1)


def cubic_lattice(n=5):
    g = np.arange(n, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def sheet(n=70001, width=301, seed=5):
    """A pixel-ordered wavy surface with a little noise, like a fused cloud: n points, ``width`` to a row, 1 cm apart."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    x, y = (i % width) * 0.01, (i // width) * 0.01
    z = 0.05 * np.sin(3.0 * x) * np.cos(2.0 * y) + 0.0005 * rng.normal(size=n)
    return np.stack([x, y, z], axis=1).astype(np.float32)


def sphere_views(points, kind):
    """``(viewpoints, view)`` of the sphere cases: none, one viewpoint, three with a ``view`` array that has unknown (-1) entries."""
    if kind == "none":
        return None, None
    if kind == "one":
        return np.array([[0.5, -3.0, 2.0]], np.float32), None
    rng = np.random.default_rng(7)
    view = rng.integers(0, 3, size=len(points)).astype(np.int32)
    view[::11] = -1
    return np.array([[4.0, 0.0, 0.0], [0.0, -4.0, 1.0], [0.1, 0.2, 0.0]], np.float32), view


def search_cases():
    """name -> (points, neighbours, max_distance, viewpoints, view)."""
    cases = {}
    points, _ = sphere()
    for k in (3, 8, 20, 32):
        for limit_name, limit in (("unbounded", np.inf), ("bounded", 0.25)):          # 0.25: short rows at k = 20 and 32
            for kind in ("none", "one", "three"):
                cases[f"sphere-k{k}-{limit_name}-{kind}"] = (points, k, limit) + sphere_views(points, kind)
    for n in (1, 2, 3, 63, 64, 65, 255, 256, 257):
        cloud = np.random.default_rng(100 + n).normal(size=(n, 3)).astype(np.float32)
        for k in (3, 8):
            cases[f"gaussian-n{n}-k{k}"] = (cloud, k, np.inf, np.array([[0.0, 0.0, 9.0]], np.float32), None)
    one = np.array([[3.0, 2.0, 10.0]], np.float32)
    cases["planar-lattice"] = (planar_lattice(), 9, np.inf, None, None)
    cases["cubic-lattice"] = (cubic_lattice(), 7, np.inf, one, None)
    cases["duplicates"] = (np.tile(np.array([[1.5, -2.25, 3.0]], np.float32), (77, 1)), 8, np.inf, one, None)
    t = np.random.default_rng(3).uniform(-2, 2, size=(300, 1))
    cases["collinear"] = ((np.array([1.0, 2.0, -1.0]) + t * np.array([0.6, -0.3, 0.7])).astype(np.float32), 8, np.inf, one, None)
    cases["tilted-plane"] = (far_plane(400, seed=2, thickness=0.0)[0], 12, np.inf, None, None)
    rng = np.random.default_rng(4)
    blob = np.concatenate([0.05 * rng.normal(size=(400, 3)), 5.0 + 3.0 * rng.uniform(size=(20, 3)) * np.arange(1, 21)[:, None]])
    cases["blob-and-far-points"] = (blob.astype(np.float32), 8, 0.5, one, None)
    return cases


def row_cases():
    """name -> (points, target, index, viewpoints, view)."""
    from dvmvs.outliers import nearest_neighbours
    cases = {}
    rng = np.random.default_rng(11)
    queries, targets = rng.normal(size=(257, 3)).astype(np.float32), rng.normal(size=(129, 3)).astype(np.float32)
    view = rng.integers(-1, 3, size=257).astype(np.int32)                 # -1 and 2 = V are unknown
    cases["separate-clouds"] = (queries, targets, nearest_neighbours(queries, targets, 10)[1],
                                np.array([[0.0, 0.0, 5.0], [5.0, 0.0, 0.0]], np.float32), view)
    # hand-made rows: -1 in the middle, and values outside [0, M): M, 2^31 - 1, -7
    M = 50
    targets = rng.normal(size=(M, 3)).astype(np.float32)
    index = rng.integers(0, M, size=(40, 8)).astype(np.int32)
    index[0:10, 3] = -1
    index[5:15, 0] = M                                                    # the anchor is then the first slot that IS valid
    index[12:20, 5] = 2 ** 31 - 1
    index[18:26, 1] = -7
    index[26, :6] = -1                                                    # two valid slots: invalid
    index[27, :] = -1
    index[28, 1:] = M + 3
    index[29] = index[29, 0]                                              # one target eight times: coincident
    cases["hand-made-rows"] = (rng.normal(size=(40, 3)).astype(np.float32), targets, index, np.array([[0.0, 1.0, 3.0]], np.float32), None)
    return cases

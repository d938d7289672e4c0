"""The meshes and clouds of the surface-sampling and voxel down-sampling tests (tests/test_surface_sample_reference.py on the host,
tests/test_surface_sample_gpu.py on the device): made once per process, never modified."""
import functools

import numpy as np


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def unit_square():
    """The unit square in the plane z = 0 as two triangles."""
    return f32([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]]), np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def grid_square(n=16):
    """The same square as an n x n grid of 2 n n triangles."""
    ticks = np.linspace(0.0, 1.0, n + 1)
    x, y = np.meshgrid(ticks, ticks, indexing="ij")
    verts = f32(np.stack([x.ravel(), y.ravel(), np.zeros(x.size)], axis=1))
    i, j = (a.ravel() for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    v00, v10, v11, v01 = i * (n + 1) + j, (i + 1) * (n + 1) + j, (i + 1) * (n + 1) + j + 1, i * (n + 1) + j + 1
    faces = np.concatenate([np.stack([v00, v10, v11], axis=1), np.stack([v00, v11, v01], axis=1)]).astype(np.int32)
    return verts, faces


@functools.lru_cache(maxsize=None)
def soup():
    """300 normal vertices, 1000 random faces, every seventh degenerate (two equal corners): 149 faces without area (six more by chance)."""
    rng = np.random.default_rng(0)
    verts = f32(rng.normal(size=(300, 3)))
    faces = rng.integers(0, 300, (1000, 3)).astype(np.int32)
    faces[::7, 1] = faces[::7, 0]
    return verts, faces


@functools.lru_cache(maxsize=None)
def small_triangles(F, seed=1):
    """F triangles of about 0.04 m^2 around random centres: about 11 samples each at density 300."""
    rng = np.random.default_rng(seed + F)
    centres = rng.uniform(-5.0, 5.0, (F, 1, 3))
    verts = f32((centres + rng.normal(size=(F, 3, 3)) * 0.15).reshape(-1, 3))
    return verts, np.arange(3 * F, dtype=np.int32).reshape(F, 3)


@functools.lru_cache(maxsize=None)
def one_large_among_tiny():
    """1000 triangles that get zero or one sample at density 100 and, in their middle, one of 2000 m^2 that gets about 200 000."""
    rng = np.random.default_rng(5)
    centres = rng.uniform(-3.0, 3.0, (1000, 1, 3))
    tiny = (centres + rng.normal(size=(1000, 3, 3)) * 0.03).reshape(-1, 3)
    verts = f32(np.concatenate([tiny, [[-20.0, -30.0, 1.0], [60.0, -30.0, 1.5], [-20.0, 20.0, 0.5]]]))
    faces = np.arange(3000, dtype=np.int32).reshape(1000, 3)
    faces = np.concatenate([faces[:500], [[3000, 3001, 3002]], faces[500:]]).astype(np.int32)
    return verts, faces


@functools.lru_cache(maxsize=None)
def out_of_range_mesh():
    """The unit square plus faces that name the vertices -1 and V: those are ignored."""
    verts, faces = unit_square()
    return verts, np.concatenate([[[0, 1, -1]], faces[:1], [[4, 1, 2], [0, 4, 3]], faces[1:], [[2, 3, 2 ** 31 - 1]]]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def speck():
    """A triangle of 5e-7 m^2: less than half a sample's share of area at density 1e6."""
    return f32([[0, 0, 0], [1e-3, 0, 0], [0, 1e-3, 0]]), np.array([[0, 1, 2]], dtype=np.int32)


def gaussian(n, seed):
    return f32(np.random.default_rng(seed).normal(size=(n, 3)))


@functools.lru_cache(maxsize=None)
def coincident(n=20000):
    return f32(np.tile([[0.3, -1.7, 2.9]], (n, 1)))


@functools.lru_cache(maxsize=None)
def on_voxel_faces(voxel=0.25):
    """Points on multiples of the voxel (counted from the cloud's minimum, the first point) and one float32 step either side of them."""
    base = f32([-1.0, 0.5, 3.0])
    steps = np.arange(0, 9, dtype=np.float32) * np.float32(voxel)
    pts = [base]
    for a in range(3):
        for s in steps[1:]:
            x = np.float32(base[a] + s)
            for value in (np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))):
                p = base.copy()
                p[a] = value
                p[(a + 1) % 3] += np.float32(0.1)
                pts.append(p)
    return f32(np.stack(pts))


@functools.lru_cache(maxsize=None)
def negative_cloud():
    return f32(np.random.default_rng(9).uniform(-7.0, -2.0, (5000, 3)))


def cell_of(points, voxel):
    """The cell the float32 formula gives, written out independently of dvmvs.errors: int32((x - mn) * float32(1 / voxel))."""
    points = f32(points)
    mn = points.min(axis=0)
    inv = np.float32(1.0 / np.float64(voxel))
    return np.trunc(np.multiply(np.subtract(points, mn, dtype=np.float32), inv, dtype=np.float32)).astype(np.int64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)

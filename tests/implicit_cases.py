"""The clouds and grids that tests/test_implicit_reference.py (CPU: vectorised host form against the scalar loop, derived properties) and
tests/test_implicit_gpu.py (device against host form) both run: numpy only, every case seeded, the smallest shapes at which the kernels can
still go wrong.  A case is a dict ``points, normals, origin, voxel, dims, radius, neighbours, min_neighbours``; ``host_volume(name)``
is its dense host result, computed once per process and shared."""
import functools

import numpy as np

PLANE_C = np.float32(0.3125)
SPHERE_R, SPHERE_VOXEL, SPHERE_RADIUS = 0.5, 0.05, 0.15


def unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def random_cloud(n, seed, low=(0.0, 0.0, 0.0), high=(1.0, 0.8, 0.6)):
    """``n`` points in a box with random unit normals."""
    rng = np.random.default_rng(seed)
    points = rng.uniform(low, high, size=(n, 3)).astype(np.float32)
    return points, unit(rng.normal(size=(n, 3))).astype(np.float32)


def wavy_sheet(n, seed, box=(1.0, 0.8)):
    """``n`` points on a gently curved sheet with its own normals, turned up."""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(0.0, box[0], size=n), rng.uniform(0.0, box[1], size=n)
    z = 0.3 + 0.05 * np.sin(4.0 * x) * np.cos(3.0 * y)
    normals = unit(np.stack([-0.2 * np.cos(4.0 * x) * np.cos(3.0 * y), 0.15 * np.sin(4.0 * x) * np.sin(3.0 * y), np.ones(n)], axis=1))
    return np.stack([x, y, z], axis=1).astype(np.float32), normals.astype(np.float32)


def plane_patch(n=12, spacing=0.05, c=PLANE_C):
    """A regular ``n`` x ``n`` patch on z = c with normals (0, 0, 1)."""
    g = (np.arange(n) * spacing).astype(np.float32)
    x, y = np.meshgrid(g, g, indexing="ij")
    points = np.stack([x.ravel(), y.ravel(), np.full(n * n, c, np.float32)], axis=1).astype(np.float32)
    return points, np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (n * n, 1))


def fibonacci_sphere(n=4000, R=SPHERE_R):
    """``n`` points on a sphere of radius ``R`` about the origin with their exact normals."""
    i = np.arange(n) + 0.5
    z = 1.0 - 2.0 * i / n
    phi = i * np.pi * (3.0 - np.sqrt(5.0))
    s = np.sqrt(1.0 - z * z)
    d = np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1)
    return (R * d).astype(np.float32), d.astype(np.float32)


def case(points, normals, origin, voxel, dims, radius, neighbours=32, min_neighbours=3):
    return dict(points=points, normals=normals, origin=np.asarray(origin, np.float32), voxel=voxel, dims=tuple(dims), radius=radius,
                neighbours=neighbours, min_neighbours=min_neighbours)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case."""
    from dvmvs.implicit import grid_for
    out = {}
    small = dict(origin=(-0.1, -0.1, -0.1), voxel=0.15, dims=(9, 7, 5), radius=0.35)         # 315 nodes: more than one workgroup
    for n in (1, 2, 63, 64, 65, 1000):
        points, normals = random_cloud(n, 10 + n)
        out[f"cloud-n{n}-9x7x5"] = case(points, normals, **small, neighbours=8, min_neighbours=1 if n < 3 else 3)
    points, normals = wavy_sheet(1000, 3)
    large = dict(origin=(-0.06, -0.05, 0.0), voxel=0.035, dims=(33, 17, 12), radius=0.09)    # 6732 nodes, a band of a few thousand
    for k in (1, 8, 31, 32):
        out[f"sheet-k{k}-33x17x12"] = case(points, normals, **large, neighbours=k, min_neighbours=1 if k == 1 else 3)
    out["thin-x-1x9x7"] = case(points, normals, (0.5, -0.05, 0.1), 0.06, (1, 9, 7), 0.15)
    out["thin-z-9x7x1"] = case(points, normals, (0.0, 0.0, 0.3), 0.1, (9, 7, 1), 0.2)
    points, normals = plane_patch()
    out["plane"] = case(points, normals, (-0.1, -0.1, 0.1), 0.05, (16, 16, 9), 0.125)
    points, normals = fibonacci_sphere()
    origin, dims = grid_for(points, SPHERE_VOXEL, SPHERE_RADIUS)
    out["sphere"] = case(points, normals, origin, SPHERE_VOXEL, dims, SPHERE_RADIUS)
    # d2 == radius^2 exactly: points at node positions shifted by exactly 0.5 along one axis, both ways; the node is a candidate of
    # weight 0 (every number here is a small multiple of 0.25: nothing rounds)
    nodes = np.array([[4, 3, 2], [1, 1, 1], [7, 5, 3], [0, 0, 0], [8, 6, 4]], np.float32) * np.float32(0.25)
    shifts = np.concatenate([np.eye(3), -np.eye(3)]).astype(np.float32) * np.float32(0.5)
    points = (nodes[:, None, :] + shifts[None, :, :]).reshape(-1, 3).astype(np.float32)
    normals = unit(np.random.default_rng(5).normal(size=(len(points), 3))).astype(np.float32)
    out["exact-boundary"] = case(points, normals, (0.0, 0.0, 0.0), 0.25, (9, 7, 5), 0.5, neighbours=32, min_neighbours=1)
    # points outside the grid on every side
    points, normals = random_cloud(600, 21, low=(-0.5, -0.5, -0.5), high=(1.5, 1.3, 1.1))
    out["points-outside"] = case(points, normals, **small, neighbours=8)
    # normals: zeros mixed in, all zero, and min_neighbours at and one above the number of used slots
    points, normals = random_cloud(400, 22)
    mixed = normals.copy()
    mixed[::3] = 0.0
    mixed[1::7] = -0.0
    out["normals-mixed-zero"] = case(points, mixed, **small, neighbours=8)
    out["normals-all-zero"] = case(points, np.zeros_like(normals), **small, neighbours=8)
    five = (np.array([[0.5, 0.35, 0.2]]) + 0.01 * np.random.default_rng(23).normal(size=(6, 3))).astype(np.float32)
    five_normals = np.tile(np.array([[0.0, 0.6, 0.8]], np.float32), (6, 1))
    five_normals[2] = 0.0                                                                     # six points, five with a normal
    out["five-used-min5"] = case(five, five_normals, **small, neighbours=8, min_neighbours=5)
    out["five-used-min6"] = case(five, five_normals, **small, neighbours=8, min_neighbours=6)
    # a radius below half a voxel: few nodes have a candidate, or none
    points, normals = random_cloud(300, 24)
    out["small-radius"] = case(points, normals, (-0.1, -0.1, -0.1), 0.15, (9, 7, 5), 0.04, neighbours=8, min_neighbours=1)
    out["tiny-radius"] = case(points[:20], normals[:20], (-0.1, -0.1, -0.1), 0.15, (9, 7, 5), 1e-4, neighbours=8, min_neighbours=1)
    return out


def arguments(c):
    """The case as the positional arguments of ``implicit_volume``."""
    return c["points"], c["normals"], c["origin"], c["voxel"], c["dims"], c["radius"], c["neighbours"], c["min_neighbours"]


@functools.lru_cache(maxsize=None)
def host_volume(name):
    """``implicit_volume`` of the case on the host, dense: computed once, shared, read-only."""
    from dvmvs.implicit import implicit_volume
    volume, valid = implicit_volume(*arguments(cases()[name]))
    volume.setflags(write=False)
    valid.setflags(write=False)
    return volume, valid

"""The scene of the sparse TSDF volume's tests (tests/test_sparse_reference.py, tests/test_sparse_volume_gpu.py): the six views, K and
frames of tests/tsdf_fuse_scene.py at 24 x 32, on a lattice with voxel 1/16 and origin (-1, -0.75, 0).  Both are dyadic, so
origin + float(v) * voxel is exact and a dense volume placed on the brick lattice reproduces a sparse voxel's position bit for bit,
negative coordinates included."""
import numpy as np

import tsdf_fuse_scene as scene

VOXEL = 1.0 / 16.0
ORIGIN = np.array([-1.0, -0.75, 0.0], dtype=np.float32)
TRUNC = 5 * VOXEL
K = scene.K
HEIGHT, WIDTH = scene.HEIGHT, scene.WIDTH
POSE_NAMES = scene.POSE_NAMES
MAX_DEPTHS = (5.0, 1.4)
# the box of the dense yardsticks, in bricks, both ends included: the "far" view reaches bricks at z = -10
BOX_FIRST = np.array([-6, -6, -14])
BOX_LAST = np.array([10, 10, 10])
BOX_BRICKS = BOX_LAST - BOX_FIRST + 1
BOX_DIMS = tuple(int(d) for d in BOX_BRICKS * 8)
BOX_ORIGIN = (ORIGIN.astype(np.float64) + BOX_FIRST * 8 * VOXEL).astype(np.float32)      # exact


def poses():
    return scene.poses()


def frames():
    """(depth [6,24,32] float32, rgb [6,24,32,3] uint8)"""
    return scene.frames(6, HEIGHT, WIDTH)


def clamp(depth, max_depth):
    d = np.array(depth, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        d[d > np.float32(max_depth)] = 0.0
    return d


def box_bounds():
    """The box in metres, [[x0,x1],[y0,y1],[z0,z1]] (exact)."""
    lo = ORIGIN.astype(np.float64) + BOX_FIRST * 8 * VOXEL
    return np.stack([lo, lo + BOX_BRICKS * 8 * VOXEL], axis=1)


def bricks_in_box(coords):
    """Mask of the brick coordinates [n,3] that lie in the box."""
    c = np.asarray(coords).reshape(-1, 3)
    return ((c >= BOX_FIRST) & (c <= BOX_LAST)).all(axis=1)


def brick_mask(coords):
    """[BOX_DIMS] bool: True in the voxels of the bricks ``coords`` [n,3] (those inside the box)."""
    c = np.asarray(coords).reshape(-1, 3)
    c = c[bricks_in_box(c)] - BOX_FIRST
    bricks = np.zeros(tuple(int(b) for b in BOX_BRICKS), dtype=bool)
    bricks[c[:, 0], c[:, 1], c[:, 2]] = True
    return np.repeat(np.repeat(np.repeat(bricks, 8, axis=0), 8, axis=1), 8, axis=2)


def planted_depth(depth):
    """A copy of one depth map [24,32] with the pixels that must mark nothing planted in its first row: 0, -0.5, NaN, +inf, -inf, and one
    above every max_depth of the tests (50)."""
    d = np.array(depth, dtype=np.float32)
    d[0, :6] = [0.0, -0.5, np.nan, np.inf, -np.inf, 50.0]
    return d

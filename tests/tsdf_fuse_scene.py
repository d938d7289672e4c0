"""The small scene of the batched TSDF fusion tests (tests/test_tsdf_fuse.py, tests/test_tsdf_fuse_gpu.py): a volume whose dimensions
(37, 30, 43) are ragged against every tile shape of csrc/tsdf_fuse.hip, and six views that exercise each plane of its culling test."""
import numpy as np

BOUNDS = np.array([[-1.0, 0.85], [-0.8, 0.65], [0.0, 2.15]])
VOXEL = 0.05
DIMS = (37, 30, 43)
HEIGHT, WIDTH = 24, 32
K = np.array([[30.0, 0.0, 15.5], [0.0, 30.0, 11.5], [0.0, 0.0, 1.0]], dtype=np.float32)
POSE_NAMES = ("front", "inside", "away", "graze", "tilt", "far")


def translation(x, y, z):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    return m


def _rotation(rows):
    m = np.eye(4)
    m[:3, :3] = rows
    return m


def rot_x(a):
    c, s = np.cos(a), np.sin(a)
    return _rotation([[1, 0, 0], [0, c, -s], [0, s, c]])


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return _rotation([[c, 0, -s], [0, 1, 0], [s, 0, c]])


def rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return _rotation([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def poses():
    """[6,4,4] float32 camera-to-world: front; inside (the camera plane cuts the volume); away (everything behind the camera); graze (a
    side of the frustum clips a corner); tilt; far (everything beyond the largest depth + truncation)."""
    return np.stack([translation(0, 0, -0.4), translation(0.1, -0.1, 0.9) @ rot_y(0.6), translation(0, 0, -0.5) @ rot_y(np.pi),
                     translation(-1.4, 0, 1.0), translation(0.3, 0.2, -0.2) @ rot_x(0.4) @ rot_z(0.7),
                     translation(0, 0, -6.0)]).astype(np.float32)


def frames(n=6, height=HEIGHT, width=WIDTH, seed=0):
    """(depth [n,h,w] float32, rgb [n,h,w,3] uint8): depth 1.3 + 0.3 sin(x / 5) + 0.2 cos(y / 4) with 10 % of the pixels 0 (a new draw
    per frame) and random colours."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width]
    base = (1.3 + 0.3 * np.sin(x / 5) + 0.2 * np.cos(y / 4)).astype(np.float32)
    depth, rgb = [], []
    for _ in range(n):
        d = base.copy()
        d[rng.random((height, width)) < 0.1] = 0.0
        depth.append(d)
        rgb.append(rng.integers(0, 256, (height, width, 3)).astype(np.uint8))
    return np.stack(depth), np.stack(rgb)


def scaled_K(height, width):
    """K for another image size of the same field of view."""
    k = K.copy()
    k[0] *= width / float(WIDTH)
    k[1] *= height / float(HEIGHT)
    return k

"""The culling test of batched TSDF fusion (``fuse_keep`` in csrc/tsdf_fuse.hip), restated in numpy with the same float64 expressions and
run on the CPU against the oracle's masks of updated voxels: a (tile, frame) pair that the test drops must hold no voxel the per-frame
update touches.  This checks the DERIVATION of the margins (the planes, the error terms, the cases of the camera plane and of non-finite
depths) over more poses than the GPU tests fuse; that the HIP code computes what is written here is what the bit-identity tests of
tests/test_tsdf_fuse_gpu.py check."""
import numpy as np
import pytest

import tsdf_fuse_scene as scene
import tsdf_oracle as tso

TILES = ((4, 4, 32), (8, 8, 8), (2, 2, 64))
ORIGIN = scene.BOUNDS[:, 0].astype(np.float32)
TRUNC = np.float32(5 * scene.VOXEL)


def frame_zmax(depth, max_depth=np.inf):
    """tsdf_fuse_zmax_kernel: the largest depth after the clamp over the pixels with depth != 0; +inf if one is not finite, -inf if none."""
    d = np.asarray(depth, dtype=np.float32).copy()
    d[d > max_depth] = 0.0
    d = d[d != 0.0]                                   # keeps NaN
    if d.size == 0:
        return -np.inf
    return np.inf if not np.isfinite(d).all() else float(d.max())


def keep(v0, n, K, pose, zmax, im_h, im_w):
    """fuse_keep, line by line: can a voxel of the tile [v0, v0 + n) pass the frame's per-voxel tests?"""
    eps = 2.0 ** -23
    K, P = np.asarray(K, dtype=np.float32).astype(np.float64), np.asarray(pose, dtype=np.float32).astype(np.float64)
    fx, cx, fy, cy = K[0, 0], K[0, 2], K[1, 1], K[1, 2]
    s = float(np.float32(scene.VOXEL))
    o = ORIGIN.astype(np.float64)
    R, t = P[:3, :3], P[:3, 3]
    h = 0.5 * (np.asarray(n, dtype=np.float64) - 1.0) * s
    c = (o + np.asarray(v0, dtype=np.float64) * s + h) - t
    B = np.abs(o) + np.asarray(scene.DIMS, dtype=np.float64) * s + np.abs(t)
    C = np.array([R[0, k] * c[0] + R[1, k] * c[1] + R[2, k] * c[2] for k in range(3)])
    H = np.array([abs(R[0, k]) * h[0] + abs(R[1, k]) * h[1] + abs(R[2, k]) * h[2] for k in range(3)])
    E = np.array([8.0 * eps * (abs(R[0, k]) * B[0] + abs(R[1, k]) * B[1] + abs(R[2, k]) * B[2]) + 1e-37 for k in range(3)])
    if C[2] + H[2] < -E[2]:
        return False                                   # behind the camera
    if C[2] - H[2] - E[2] > zmax + float(TRUNC) * (1.0 + 4.0 * eps):
        return False                                   # beyond zmax + truncation
    if C[2] - H[2] > E[2]:                             # wholly in front: the four image sides
        for k, (focal, centre, size) in enumerate(((fx, cx, float(im_w)), (fy, cy, float(im_h)))):
            S = size + abs(centre) + 1.0
            mu = 6.0 * eps * S + (abs(focal) + 1.0) * 1e-37
            a_hi, a_lo = size - 0.5 - centre + mu, -0.5 - centre - mu
            hi_c, lo_c = focal * C[k] - a_hi * C[2], focal * C[k] - a_lo * C[2]
            hi_h = sum(abs(focal * R[a, k] - a_hi * R[a, 2]) * h[a] for a in range(3))
            lo_h = sum(abs(focal * R[a, k] - a_lo * R[a, 2]) * h[a] for a in range(3))
            if hi_c - hi_h > abs(focal) * E[k] + abs(a_hi) * E[2]:
                return False
            if lo_c + lo_h < -(abs(focal) * E[k] + abs(a_lo) * E[2]):
                return False
    return True


def updated(depth, pose, K=scene.K):
    """The oracle's mask of voxels that one frame updates."""
    vols = [np.ones(scene.DIMS, np.float32), np.zeros(scene.DIMS, np.float32), np.zeros(scene.DIMS, np.float32)]
    return tso.integrate(*vols, ORIGIN, scene.VOXEL, K, pose, np.zeros_like(depth), depth, TRUNC)


def tiles_of(tile):
    for x0 in range(0, scene.DIMS[0], tile[0]):
        for y0 in range(0, scene.DIMS[1], tile[1]):
            for z0 in range(0, scene.DIMS[2], tile[2]):
                v0 = (x0, y0, z0)
                yield v0, tuple(min(tile[a], scene.DIMS[a] - v0[a]) for a in range(3))


def check(depth, pose, tile, K=scene.K, max_depth=np.inf):
    """(pairs kept, tiles that hold an updated voxel) of one frame; asserts that no such tile is dropped."""
    clamped = np.asarray(depth, dtype=np.float32).copy()
    clamped[clamped > max_depth] = 0.0
    mask = updated(clamped, pose, K)
    zmax = frame_zmax(depth, max_depth)
    kept = needed = 0
    for v0, n in tiles_of(tile):
        holds = bool(mask[v0[0]:v0[0] + n[0], v0[1]:v0[1] + n[1], v0[2]:v0[2] + n[2]].any())
        stays = keep(v0, n, K, pose, zmax, *depth.shape)
        assert stays or not holds, f"tile at {v0} of shape {tile} holds an updated voxel and is dropped"
        kept += stays
        needed += holds
    return kept, needed


def random_poses(n, seed=11):
    """Cameras in and around the volume: every other one looks anywhere (a rotation from a random unit quaternion), the others roughly
    at the volume's centre, so that many of them update voxels."""
    rng = np.random.RandomState(seed)
    centre, extent = scene.BOUNDS.mean(axis=1), scene.BOUNDS[:, 1] - scene.BOUNDS[:, 0]
    out = []
    for i in range(n):
        m = np.eye(4)
        m[:3, 3] = centre + rng.uniform(-1.0, 1.0, 3) * extent
        if i % 2:
            w, x, y, z = (lambda q: q / np.linalg.norm(q))(rng.normal(size=4))
            m[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
        else:
            forward = centre + rng.uniform(-0.3, 0.3, 3) * extent - m[:3, 3]
            forward /= np.linalg.norm(forward)
            right = np.cross(rng.normal(size=3), forward)
            right /= np.linalg.norm(right)
            m[:3, :3] = np.stack([right, np.cross(forward, right), forward], axis=1)      # columns: the camera's x, y, z axes in the world
        out.append(m.astype(np.float32))
    return out


@pytest.mark.parametrize("tile", TILES)
def test_no_tile_with_an_updated_voxel_is_dropped_on_the_six_views(tile):
    depth, _ = scene.frames()
    n_tiles = len(list(tiles_of(tile)))
    counts = {name: check(d, pose, tile) for name, d, pose in zip(scene.POSE_NAMES, depth, scene.poses())}
    assert counts["away"] == (0, 0) and counts["far"] == (0, 0)             # dropped everywhere, and rightly
    for name in ("front", "inside", "tilt", "graze"):
        kept, needed = counts[name]
        assert 0 < needed <= kept <= n_tiles, (name, kept, needed)
    # a view that clips one corner keeps only some tiles -- unless every tile spans the volume in z: "graze" looks along z from z = 1.0,
    # its camera plane then cuts every tile, and a tile that the camera plane cuts is never dropped by a side plane
    assert counts["graze"][0] < n_tiles or tile[2] >= scene.DIMS[2]


@pytest.mark.parametrize("tile", TILES)
def test_no_tile_with_an_updated_voxel_is_dropped_on_random_views(tile):
    depth, _ = scene.frames(5, seed=4)
    n_tiles = len(list(tiles_of(tile)))
    kept = needed = views_that_update = 0
    for i, pose in enumerate(random_poses(30)):
        k, m = check(depth[i % 5], pose, tile, max_depth=(np.inf, 1.4)[i % 3 == 0])
        kept, needed, views_that_update = kept + k, needed + m, views_that_update + (m > 0)
    print(f"tile {tile}: {views_that_update} of 30 views update voxels; {needed} tiles hold one, {kept} of {30 * n_tiles} pairs kept")
    assert views_that_update >= 10 and needed <= kept < 30 * n_tiles          # not vacuous, and it culls


def test_frames_without_a_far_plane_and_without_a_pixel():
    """A NaN or infinite depth is integrated with dist = 1 all along its ray, so the frame has no far plane: from the "far" pose, which a
    finite frame cannot reach, the NaN pixel's ray updates voxels, and their tiles stay.  A frame of zeros drops every tile."""
    depth, _ = scene.frames()
    far = scene.poses()[5]
    for bad in (np.nan, np.inf):
        d = depth[0].copy()
        d[12, 16] = bad
        assert frame_zmax(d) == np.inf
        kept, needed = check(d, far, TILES[0])
        assert needed > 0 and kept >= needed
    zeros = np.zeros_like(depth[0])
    assert frame_zmax(zeros) == -np.inf and check(zeros, scene.poses()[0], TILES[0]) == (0, 0)
    assert frame_zmax(depth[0], max_depth=0.5) == -np.inf                  # every pixel above the clamp

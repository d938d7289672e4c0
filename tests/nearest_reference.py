"""Test reference of the nearest-point op and the 3-D reconstruction metrics (csrc/nearest_points.hip, dvmvs.errors), restated twice:
``nearest64`` is the float64 brute force (the truth the float32 contract is measured against), ``nearest32`` the float32 formula of the
contract -- ``sqrt(min_j (dx*dx + dy*dy) + dz*dz)`` -- with dx, dy, dz as separate numpy arrays, so that every operation is one
elementwise numpy call that rounds to float32 and nothing can be fused.  Written independently of dvmvs.errors, which the tests compare
with it."""
import math

import numpy as np

NAMES = ("acc", "comp", "chamfer", "precision", "recall", "fscore")
# |d32 - d64| <= 4 * 2^-24 * d64: along the chain subtraction, product, sum, sum a component of d^2 collects at most five roundings
# (the subtraction's counts twice, it is squared), 5 * 2^-24 relative on d^2; half of that passes through the square root, and the root
# adds its own rounding: 3.5 * 2^-24, rounded up to 4
ERROR_BOUND = 4.0 * 2.0 ** -24


def _chunks(n_query, n_target, pairs=1 << 22):
    step = max(1, pairs // max(n_target, 1))
    return [(b, min(b + step, n_query)) for b in range(0, n_query, step)]


def nearest64(query, target):
    """float64 [N]: exact (to float64) distance to the nearest target, and int64 [N] the smallest index of one."""
    q, t = np.asarray(query, dtype=np.float64), np.asarray(target, dtype=np.float64)
    dist, index = np.empty(len(q)), np.empty(len(q), dtype=np.int64)
    for b, e in _chunks(len(q), len(t)):
        d2 = ((q[b:e, None, :] - t[None, :, :]) ** 2).sum(axis=2)
        index[b:e] = np.argmin(d2, axis=1)
        dist[b:e] = np.sqrt(d2[np.arange(e - b), index[b:e]])
    return dist, index


def nearest32(query, target):
    """float32 [N] and int32 [N]: the contract's float32 formula by brute force; the smallest index among equal minima."""
    q, t = np.asarray(query, dtype=np.float32), np.asarray(target, dtype=np.float32)
    assert q.dtype == np.float32 and t.dtype == np.float32
    tx, ty, tz = t[:, 0].copy(), t[:, 1].copy(), t[:, 2].copy()
    dist, index = np.empty(len(q), dtype=np.float32), np.empty(len(q), dtype=np.int32)
    for b, e in _chunks(len(q), len(t)):
        dx = np.subtract(q[b:e, 0][:, None], tx[None, :])
        dy = np.subtract(q[b:e, 1][:, None], ty[None, :])
        dz = np.subtract(q[b:e, 2][:, None], tz[None, :])
        xx, yy, zz = np.multiply(dx, dx), np.multiply(dy, dy), np.multiply(dz, dz)
        d2 = np.add(np.add(xx, yy), zz)
        assert d2.dtype == np.float32
        nearest = np.argmin(d2, axis=1)                    # numpy returns the first occurrence
        index[b:e] = nearest
        dist[b:e] = np.sqrt(d2[np.arange(e - b), nearest])
    return dist, index


def metrics(dist_pred, dist_gt, threshold):
    """(float32 [6], int64 [2]) from the two float32 distance arrays: exact sums (fsum), every entry rounded to float32 once."""
    threshold = np.float32(threshold)
    acc = math.fsum(map(float, dist_pred)) / len(dist_pred)
    comp = math.fsum(map(float, dist_gt)) / len(dist_gt)
    below = [int((dist_pred < threshold).sum()), int((dist_gt < threshold).sum())]
    p, r = below[0] / len(dist_pred), below[1] / len(dist_gt)
    f = 2.0 * p * r / (p + r) if p + r > 0.0 else 0.0
    return np.array([acc, comp, (acc + comp) / 2.0, p, r, f], dtype=np.float32), np.array(below, dtype=np.int64)


def reconstruction_errors(pred, gt, threshold):
    return metrics(nearest32(pred, gt)[0], nearest32(gt, pred)[0], threshold)


def ulps(a, b):
    """Distance in float32 representable numbers between two non-negative float32 arrays."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ---- the hand-computed clouds shared by the CPU and the GPU tests: (name, pred, gt, threshold, expected row) -----------------------------
def hand_cases():
    g = np.arange(4, dtype=np.float32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    shifted = lattice + np.array([0.25, 0.0, 0.0], dtype=np.float32)           # 0.25 and the lattice coordinates are exact in float32
    # asymmetric: the prediction is ONE point 0.1 from the first of two ground-truth points that lie 1 apart:
    # acc = 0.1 (P = 1 at 0.5); comp = (0.1 + 0.9) / 2 = 0.5 (R = 1/2); F = 2 * 1 * 0.5 / 1.5 = 2/3
    pred = np.array([[0.1, 0.0, 0.0]], dtype=np.float32)
    gt = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], dtype=np.float32)
    d_near, d_far = float(np.float32(0.1)), float(np.float32(1.0) - np.float32(0.1))
    asym = [d_near, (d_near + d_far) / 2, (d_near + (d_near + d_far) / 2) / 2, 1.0, 0.5, 2.0 / 3.0]
    return [("identical", lattice, lattice.copy(), 0.05, [0, 0, 0, 1, 1, 1]),
            ("shifted_0.3", lattice, shifted, 0.3, [0.25, 0.25, 0.25, 1, 1, 1]),
            ("shifted_0.2", lattice, shifted, 0.2, [0.25, 0.25, 0.25, 0, 0, 0]),
            ("asymmetric", pred, gt, 0.5, asym)]

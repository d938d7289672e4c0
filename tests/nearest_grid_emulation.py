"""The grid of csrc/nearest_points.hip restated in numpy, statement for statement in float32: the header (box, cell edge, dimensions),
the cell function and the ring search with its stop rule.  tests/test_nearest_reference.py holds the emulation to the brute force on
the CPU; ``face_case`` builds, for a given header, targets that sit ON cell faces and queries one float32 step either side of them,
for the CPU test (emulated header) and the GPU test (the header the device computed)."""
import numpy as np

f = np.float32
MAX_CELLS, MAX_DIM = 1 << 22, 1024


def header(target):
    """nn_header_kernel: {'mn', 'mx', 'inv_h', 'h_lo', 'dim'} of a float32 [M,3] cloud."""
    target = np.asarray(target, dtype=f)
    capacity = min(max(4 * len(target), 64), MAX_CELLS)
    mn, mx = target.min(axis=0), target.max(axis=0)
    ext = (mx - mn).astype(f)
    emax = ext.max()
    h = {"mn": mn, "mx": mx, "inv_h": f(0), "h_lo": f(0), "dim": np.ones(3, np.int32)}
    if np.isfinite(ext).all() and f(1e-12) <= emax <= f(1e12):
        occupied = ext[ext > 0].astype(np.float64)
        per_cell = occupied.prod() / capacity
        h0 = per_cell if len(occupied) == 1 else (np.sqrt(per_cell) if len(occupied) == 2 else np.cbrt(per_cell))
        edge = max(f(h0), f(emax / f(1000)))
        for _ in range(128):
            inv = f(1) / edge
            s = (ext * inv).astype(f)
            if (s < MAX_DIM).all():
                dim = s.astype(np.int32) + 1
                if int(dim[0]) * int(dim[1]) * int(dim[2]) <= capacity:
                    h.update(inv_h=inv, h_lo=f(edge * f(0.9990234375)), dim=dim)
                    break
            edge = f(edge * f(1.125))
    return h


def scaled(h, x, axis):
    """s(x) = fl(fl(clamp(x) - mn) * inv_h) on one axis; the cell is its integer part."""
    c = np.minimum(np.maximum(np.asarray(x, dtype=f), h["mn"][axis]), h["mx"][axis])
    return ((c - h["mn"][axis]).astype(f) * h["inv_h"]).astype(f)


def cells(h, points):
    """nn_cell: int [N,3]."""
    points = np.asarray(points, dtype=f)
    k = np.stack([scaled(h, points[:, a], a).astype(np.int64) for a in range(3)], axis=1)
    return np.minimum(np.maximum(k, 0), h["dim"].astype(np.int64) - 1)


def search(query, target):
    """nn_query_kernel for every query: (dist float32 [N], index int32 [N], rings searched [N])."""
    query, target = np.asarray(query, dtype=f), np.asarray(target, dtype=f)
    h = header(target)
    X, Y, Z = (int(d) for d in h["dim"])
    buckets = {}
    for j, (cx, cy, cz) in enumerate(cells(h, target)):
        buckets.setdefault((cx * Y + cy) * Z + cz, []).append(j)
    dist, index, rings = np.empty(len(query), f), np.empty(len(query), np.int32), np.empty(len(query), np.int64)
    for i, (q, (cx, cy, cz)) in enumerate(zip(query, cells(h, query))):
        rmax = max(cx, X - 1 - cx, cy, Y - 1 - cy, cz, Z - 1 - cz)
        best, best_j, r = f(np.inf), 2 ** 31 - 1, 0
        while True:
            visit = []
            for x in range(max(cx - r, 0), min(cx + r, X - 1) + 1):
                for y in range(max(cy - r, 0), min(cy + r, Y - 1) + 1):
                    if abs(x - cx) == r or abs(y - cy) == r:
                        zs = range(max(cz - r, 0), min(cz + r, Z - 1) + 1)
                    else:
                        zs = [z for z in (cz - r, cz + r) if 0 <= z <= Z - 1]
                    for z in zs:
                        visit += buckets.get((x * Y + y) * Z + z, [])
            if visit:
                t = target[visit]
                dx, dy, dz = q[0] - t[:, 0], q[1] - t[:, 1], q[2] - t[:, 2]
                d2 = (dx * dx + dy * dy) + dz * dz
                for value, j in zip(d2, visit):
                    if value < best or (value == best and j < best_j):
                        best, best_j = value, j
            if r >= rmax:
                break
            rb = f(f(r) * h["h_lo"])
            if r >= 1 and best <= f(f(rb * rb) * f(0.998)):
                break
            r += 1
        dist[i], index[i], rings[i] = np.sqrt(best), best_j, r
    return dist, index, rings


def face_coordinate(h, axis, k):
    """The smallest float32 x of the box with cell k on ``axis`` (1 <= k < dim): x is ON the face between the cells k - 1 and k."""
    x = f(np.float64(h["mn"][axis]) + k / np.float64(h["inv_h"]))
    while scaled(h, x, axis) >= k:
        x = np.nextafter(x, f(-np.inf))
    while scaled(h, x, axis) < k:
        x = np.nextafter(x, f(np.inf))
    return x


FACE_BOX = (np.array([-0.3, 0.2, 1.0], dtype=f), np.array([0.9, 1.1, 1.7], dtype=f))
FACE_M = 600


def box_corners(box=FACE_BOX):
    lo, hi = box
    return np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=f)


def provisional_cloud(box=FACE_BOX, m=FACE_M, seed=31):
    """A cloud with the box and the size of the face case: they alone decide the header."""
    lo, hi = box
    inner = np.random.default_rng(seed).uniform(lo, hi, size=(m - 8, 3)).astype(f)
    return np.concatenate([box_corners(box), np.minimum(np.maximum(inner, lo), hi)])


def face_case(h, box=FACE_BOX, m=FACE_M, seed=32):
    """(query, target, face_cells): ``target`` = the box's corners and m - 8 points whose three coordinates lie ON faces of the grid ``h``
    (interior faces, drawn at random; ``face_cells`` [m - 8, 3] are their cells); ``query`` = those points, the same one float32 step
    up and down on every axis and on mixed axes, and the centres of their cells."""
    rng = np.random.default_rng(seed)
    dim = h["dim"].astype(np.int64)
    assert (dim >= 3).all(), f"the face case needs interior faces on every axis, got {dim}"
    ks = np.stack([rng.integers(1, dim[a], size=m - 8) for a in range(3)], axis=1)
    table = [{k: face_coordinate(h, a, k) for k in range(1, dim[a])} for a in range(3)]
    on_faces = np.array([[table[a][k[a]] for a in range(3)] for k in ks], dtype=f)
    target = np.concatenate([box_corners(box), on_faces])
    some = on_faces[:120]
    up, down = np.nextafter(some, f(np.inf)), np.nextafter(some, f(-np.inf))
    mixed = some.copy()
    mixed[:, 0], mixed[:, 2] = up[:, 0], down[:, 2]
    one_axis = [np.where(np.arange(3) == a, side, some) for a in range(3) for side in (up, down)]
    centres = (some + f(0.5) / h["inv_h"]).astype(f)
    return np.concatenate([some, up, down, mixed, centres] + one_axis).astype(f), target, ks


def assert_on_faces(h, on_faces, ks):
    """The premise of the face case under header ``h``: every coordinate has its cell, and one float32 step below it the cell before."""
    for a in range(3):
        x = on_faces[:, a]
        assert (scaled(h, x, a).astype(np.int64) == ks[:, a]).all()
        assert (scaled(h, np.nextafter(x, f(-np.inf)), a).astype(np.int64) == ks[:, a] - 1).all()
    assert (ks >= 1).all() and (ks < h["dim"]).all()

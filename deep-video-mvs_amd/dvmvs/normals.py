"""Oriented normals of point clouds: what a fused cloud (``dvmvs.consistency.fused_point_cloud``, cleaned by ``dvmvs.outliers``) lacks for
Poisson meshing, point-to-plane registration, normal-based filtering and shaded viewing.  The usual recipe (Open3D's ``estimate_normals``
and ``orient_normals_towards_camera_location``): the normal of a point is the eigenvector of the smallest eigenvalue of the covariance of
its k nearest neighbours, turned toward the camera that saw the point.

This module is the host definition, in numpy, importable without a GPU.  ``point_normals_device`` and ``estimate_normals_device`` are the
same on the GPU (``dvmvs.hip.normals``, csrc/point_normals.hip) and give the same bits.

Arithmetic contract (include/dvmvs_hip.h states it for the C entry): everything is float64 computed from the float32 inputs with +, -, *,
/ and sqrt only, every operation correctly rounded, nothing fused.  For point i with row ``index[i]`` of k slots:

1. The VALID slots are those with ``0 <= j < M``, in slot order: j0, j1, ..., n of them (-1 and every other value outside are skipped).
   ``n < 3``: normal (0,0,0), curvature 0, invalid.
2. Single-pass moments about the anchor ``a = target[j0]``: for every valid slot in order ``e = target[j] - a``, ``s_c += e_c``,
   ``S_cd += e_c * e_d`` for (c,d) = (0,0),(0,1),(0,2),(1,1),(1,2),(2,2), all sums from 0.0; then ``m_c = s_c / n`` and
   ``C_cd = S_cd / n - m_c * m_d``.  (The anchor is a point of the neighbourhood, so the differences are small and exact or nearly so
   wherever the cloud lies: the cancellation of a one-pass covariance about the origin does not occur, and no second pass is needed.)
3. Cyclic Jacobi on the symmetric 3x3, the rule of the registration's 4x4: pairs (p,q) = (0,1),(0,2),(1,2); a zero ``A_pq`` is skipped;
   ``theta = (A_qq - A_pp) / (2 A_pq)``, ``t = 1 / (|theta| + sqrt(theta theta + 1))`` with the sign of theta (+ for 0),
   ``c = 1 / sqrt(t t + 1)``, ``s = t c``; the columns p, q of A, then its rows, old values on the right (``new_p = c old_p - s old_q``,
   ``new_q = s old_p + c old_q``), then ``A_pq = A_qp = 0``, then the columns p, q of V (from the identity).  Before each sweep: stop when
   the three off-diagonals are exactly zero; at most 16 sweeps.
4. ``lambda`` = the smallest diagonal entry, the lowest index on a tie; ``trace = (A_00 + A_11) + A_22``.  A trace that is not > 0
   (coincident points): normal 0, curvature 0, invalid.  Otherwise ``curvature = float32(max(lambda, 0) / trace)`` and the point is valid.
5. The normal is that column of V divided by ``sqrt((x x + y y) + z z)``, negated when the first non-zero of (z, y, x) is negative.
6. With ``viewpoints``: ``v = viewpoints[view[i]]`` (``viewpoints[0]`` without ``view``, which needs V = 1; a ``view[i]`` outside [0, V) means
   unknown and keeps the sign of 5), ``d = (n_x (v_x - p_x) + n_y (v_y - p_y)) + n_z (v_z - p_z)`` with ``p = points[i]``; the normal is
   negated when ``d < 0``.  Then every component is rounded to float32.
Coordinates must be finite."""
import math

import numpy as np

from dvmvs.outliers import MAX_NEIGHBOURS, nearest_neighbours

MIN_NEIGHBOURS = 3
SWEEPS = 16
_PAIRS = ((0, 1), (0, 2), (1, 2))


def _arguments(name, points, target, index, viewpoints, view):
    """The checked arrays: float32 clouds, int64 index [N,k], float32 viewpoints [V,3] or None, int64 view [N] or None."""
    points = np.ascontiguousarray(points, dtype=np.float32)
    target = np.ascontiguousarray(target, dtype=np.float32)
    for label, cloud in (("points", points), ("target", target)):
        if cloud.ndim != 2 or cloud.shape[1] != 3:
            raise ValueError(f"{name}: {label} must be float32 [N,3], got {cloud.shape}")
    if len(target) == 0:
        raise ValueError(f"{name}: the target cloud is empty")
    index = np.asarray(index)
    if index.ndim != 2 or index.shape[0] != len(points) or not np.issubdtype(index.dtype, np.integer):
        raise ValueError(f"{name}: index must be an integer array [{len(points)},k], got {index.dtype} {index.shape}")
    if not MIN_NEIGHBOURS <= index.shape[1] <= MAX_NEIGHBOURS:
        raise ValueError(f"{name}: index must have between {MIN_NEIGHBOURS} and {MAX_NEIGHBOURS} slots a row, got {index.shape[1]}")
    index = index.astype(np.int64)
    if viewpoints is None:
        if view is not None:
            raise ValueError(f"{name}: view chooses among viewpoints: it needs viewpoints")
        return points, target, index, None, None
    viewpoints = np.ascontiguousarray(viewpoints, dtype=np.float32)
    if viewpoints.ndim != 2 or viewpoints.shape[1] != 3 or len(viewpoints) == 0:
        raise ValueError(f"{name}: viewpoints must be float32 [V,3] with V >= 1, got {viewpoints.shape}")
    if view is None:
        if len(viewpoints) != 1:
            raise ValueError(f"{name}: {len(viewpoints)} viewpoints need view, the viewpoint of every point")
        return points, target, index, viewpoints, None
    view = np.asarray(view)
    if view.shape != (len(points),) or not np.issubdtype(view.dtype, np.integer):
        raise ValueError(f"{name}: view must be an integer array [{len(points)}], got {view.dtype} {view.shape}")
    return points, target, index, viewpoints, view.astype(np.int64)


def point_normals(points, target, index, viewpoints=None, view=None):
    """``(normals float32 [N,3], curvature float32 [N], valid bool [N])`` of ``points`` float32 [N,3] from the neighbours ``index`` int [N,k]
    (3 <= k <= 32; rows of ``nearest_neighbours(points, target, k, max_distance, exclude_same_index=False)``) in ``target`` float32 [M,3],
    by the module's definition; oriented toward ``viewpoints`` float32 [V,3] (``view`` int [N] says which; without it V must be 1) when
    given.  Vectorised over the points: elementwise float64 operations of numpy are the correctly rounded ones, so the bits are those of
    the per-point loop ``_point_normals_scalar``."""
    points, target, index, viewpoints, view = _arguments("point_normals", points, target, index, viewpoints, view)
    N, k, M = len(points), index.shape[1], len(target)
    target64 = target.astype(np.float64)
    inside = (index >= 0) & (index < M)
    n = np.count_nonzero(inside, axis=1)
    first = np.argmax(inside, axis=1)                                     # the first valid slot (0 for a row without one: masked below)
    rows = np.arange(N)
    anchor = target64[np.where(inside[rows, first], index[rows, first], 0)] if N else np.zeros((0, 3))
    s = [np.zeros(N) for _ in range(3)]
    S = {cd: np.zeros(N) for cd in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))}
    for slot in range(k):
        ok = inside[:, slot]
        e = target64[np.where(ok, index[:, slot], 0)] - anchor
        for c in range(3):
            s[c] = np.where(ok, s[c] + e[:, c], s[c])
        for (c, d) in S:
            S[(c, d)] = np.where(ok, S[(c, d)] + e[:, c] * e[:, d], S[(c, d)])
    count = np.maximum(n, 1).astype(np.float64)
    m = [s[c] / count for c in range(3)]
    A = {cd: S[cd] / count - m[cd[0]] * m[cd[1]] for cd in S}             # the upper triangle: the rotations keep A symmetric bit for bit
    V = [[np.full(N, float(r == c)) for c in range(3)] for r in range(3)]
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            if not ((A[(0, 1)] != 0.0) | (A[(0, 2)] != 0.0) | (A[(1, 2)] != 0.0)).any():
                break
            for p, q in _PAIRS:
                r = 3 - p - q
                pr, qr = (min(p, r), max(p, r)), (min(q, r), max(q, r))
                turn = A[(p, q)] != 0.0                                   # a finished row has three zeros: nothing turns in it
                apq = np.where(turn, A[(p, q)], 1.0)
                theta = (A[(q, q)] - A[(p, p)]) / (2.0 * apq)
                t = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                t = np.where(theta < 0.0, -t, t)
                c = 1.0 / np.sqrt(t * t + 1.0)
                sn = t * c
                app, aqq, apq = A[(p, p)], A[(q, q)], A[(p, q)]
                # the columns p, q (rows p and q of them), then the rows p, q at k = p and k = q
                pp, pq_ = c * app - sn * apq, sn * app + c * apq
                qp, qq = c * apq - sn * aqq, sn * apq + c * aqq
                A[(p, p)] = np.where(turn, c * pp - sn * qp, app)
                A[(q, q)] = np.where(turn, sn * pq_ + c * qq, aqq)
                A[(p, q)] = np.where(turn, 0.0, apq)
                apr, aqr = A[pr], A[qr]
                A[pr] = np.where(turn, c * apr - sn * aqr, apr)
                A[qr] = np.where(turn, sn * apr + c * aqr, aqr)
                for row in range(3):
                    vp, vq = V[row][p], V[row][q]
                    V[row][p] = np.where(turn, c * vp - sn * vq, vp)
                    V[row][q] = np.where(turn, sn * vp + c * vq, vq)
        diagonal = [A[(0, 0)], A[(1, 1)], A[(2, 2)]]
        best = np.zeros(N, dtype=np.int64)
        lam = diagonal[0]
        for c in (1, 2):
            smaller = diagonal[c] < lam
            best = np.where(smaller, c, best)
            lam = np.where(smaller, diagonal[c], lam)
        trace = (diagonal[0] + diagonal[1]) + diagonal[2]
        valid = (n >= MIN_NEIGHBOURS) & (trace > 0.0)
        curvature = np.where(valid, np.where(lam > 0.0, lam, 0.0) / np.where(valid, trace, 1.0), 0.0)
        x, y, z = (np.where(best == 0, V[r][0], np.where(best == 1, V[r][1], V[r][2])) for r in range(3))
        norm = np.sqrt((x * x + y * y) + z * z)
        x, y, z = x / norm, y / norm, z / norm
        flip = (z < 0.0) | ((z == 0.0) & ((y < 0.0) | ((y == 0.0) & (x < 0.0))))
        x, y, z = np.where(flip, -x, x), np.where(flip, -y, y), np.where(flip, -z, z)
        if viewpoints is not None:
            known = np.ones(N, dtype=bool) if view is None else (view >= 0) & (view < len(viewpoints))
            v = viewpoints.astype(np.float64)[np.zeros(N, dtype=np.int64) if view is None else np.where(known, view, 0)]
            p = points.astype(np.float64)
            d = (x * (v[:, 0] - p[:, 0]) + y * (v[:, 1] - p[:, 1])) + z * (v[:, 2] - p[:, 2])
            away = known & (d < 0.0)
            x, y, z = np.where(away, -x, x), np.where(away, -y, y), np.where(away, -z, z)
        normals = np.stack([np.where(valid, x, 0.0), np.where(valid, y, 0.0), np.where(valid, z, 0.0)], axis=1).astype(np.float32)
    return normals, curvature.astype(np.float32), valid


def _jacobi3(A):
    """Cyclic Jacobi on a symmetric 3x3 (lists of Python floats): ``(diagonal, V)`` after at most 16 sweeps; step 3 of the definition."""
    A = [list(row) for row in A]
    V = [[float(r == c) for c in range(3)] for r in range(3)]
    for _ in range(SWEEPS):
        if all(A[p][q] == 0.0 for p, q in _PAIRS):
            break
        for p, q in _PAIRS:
            if A[p][q] == 0.0:
                continue
            theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q])
            t = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))
            if theta < 0.0:
                t = -t
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            for k in range(3):
                old_p, old_q = A[k][p], A[k][q]
                A[k][p] = c * old_p - s * old_q
                A[k][q] = s * old_p + c * old_q
            for k in range(3):
                old_p, old_q = A[p][k], A[q][k]
                A[p][k] = c * old_p - s * old_q
                A[q][k] = s * old_p + c * old_q
            A[p][q] = A[q][p] = 0.0
            for k in range(3):
                old_p, old_q = V[k][p], V[k][q]
                V[k][p] = c * old_p - s * old_q
                V[k][q] = s * old_p + c * old_q
    return [A[k][k] for k in range(3)], V


def _point_normals_scalar(points, target, index, viewpoints=None, view=None):
    """``point_normals`` as a loop over the points in Python floats (IEEE float64, every operation rounded on its own): the definition read
    line by line.  Slow; the tests hold ``point_normals`` equal to it bit for bit."""
    points, target, index, viewpoints, view = _arguments("point_normals", points, target, index, viewpoints, view)
    N, M = len(points), len(target)
    normals, curvature, valid = np.zeros((N, 3), np.float32), np.zeros(N, np.float32), np.zeros(N, bool)
    for i in range(N):
        slots = [int(j) for j in index[i] if 0 <= int(j) < M]
        n = len(slots)
        if n < MIN_NEIGHBOURS:
            continue
        a = [float(v) for v in target[slots[0]]]
        s = [0.0, 0.0, 0.0]
        S = [[0.0] * 3 for _ in range(3)]
        for j in slots:
            e = [float(target[j][c]) - a[c] for c in range(3)]
            for c in range(3):
                s[c] += e[c]
                for d in range(c, 3):
                    S[c][d] += e[c] * e[d]
        m = [s[c] / n for c in range(3)]
        C = [[0.0] * 3 for _ in range(3)]
        for c in range(3):
            for d in range(c, 3):
                C[c][d] = C[d][c] = S[c][d] / n - m[c] * m[d]
        diagonal, V = _jacobi3(C)
        best = 0
        for c in (1, 2):
            if diagonal[c] < diagonal[best]:
                best = c
        trace = (diagonal[0] + diagonal[1]) + diagonal[2]
        if not trace > 0.0:
            continue
        x, y, z = V[0][best], V[1][best], V[2][best]
        norm = math.sqrt((x * x + y * y) + z * z)
        x, y, z = x / norm, y / norm, z / norm
        if z < 0.0 or (z == 0.0 and (y < 0.0 or (y == 0.0 and x < 0.0))):
            x, y, z = -x, -y, -z
        if viewpoints is not None:
            which = 0 if view is None else int(view[i])
            if 0 <= which < len(viewpoints):
                v, p = [float(c) for c in viewpoints[which]], [float(c) for c in points[i]]
                if (x * (v[0] - p[0]) + y * (v[1] - p[1])) + z * (v[2] - p[2]) < 0.0:
                    x, y, z = -x, -y, -z
        normals[i] = (x, y, z)
        curvature[i] = (diagonal[best] if diagonal[best] > 0.0 else 0.0) / trace
        valid[i] = True
    return normals, curvature, valid


def _neighbours(name, neighbours):
    if isinstance(neighbours, bool) or not isinstance(neighbours, (int, np.integer)) or not MIN_NEIGHBOURS <= int(neighbours) <= MAX_NEIGHBOURS:
        raise ValueError(f"{name}: neighbours must be an integer in [{MIN_NEIGHBOURS}, {MAX_NEIGHBOURS}], got {neighbours!r}")
    return int(neighbours)


def estimate_normals(points, neighbours=20, max_distance=np.inf, viewpoints=None, view=None):
    """``(normals float32 [N,3], curvature float32 [N], valid bool [N])`` of a cloud float32 [N,3] from each point's ``neighbours`` nearest
    points within ``max_distance``, the point itself among them (``nearest_neighbours(points, points, neighbours, max_distance, False)``,
    then ``point_normals``).  A point with fewer than 3 such points, or whose neighbours all coincide, is invalid and gets a zero normal.
    ``3 <= neighbours <= 32``."""
    neighbours = _neighbours("estimate_normals", neighbours)
    points = np.ascontiguousarray(points, dtype=np.float32)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"estimate_normals: points must be float32 [N,3], got {points.shape}")
    if len(points) == 0:
        return np.zeros((0, 3), np.float32), np.zeros(0, np.float32), np.zeros(0, bool)
    _, index = nearest_neighbours(points, points, neighbours, max_distance, False)
    return point_normals(points, points, index, viewpoints, view)


def point_normals_device(points, target, index, viewpoints=None, view=None):
    """``point_normals`` for device tensors (``dvmvs.hip.normals.point_normals``): the same bits, on the GPU; nothing is read by the host."""
    from dvmvs.hip import normals
    return normals.point_normals(points, target, index, viewpoints, view)


def estimate_normals_device(points, neighbours=20, max_distance=np.inf, viewpoints=None, view=None):
    """``estimate_normals`` for a device tensor (``dvmvs.hip.normals.estimate_normals``): the same bits, on the GPU; nothing is read by the
    host."""
    from dvmvs.hip import normals
    return normals.estimate_normals(points, neighbours, max_distance, viewpoints, view)

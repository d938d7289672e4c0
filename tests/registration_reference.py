"""Test reference of the registration (csrc/registration.hip, dvmvs.errors.register_points): the contract of include/dvmvs_hip.h restated
in numpy, written independently of dvmvs.errors, which the tests compare with it.  The float32 transform with every operation a separate
numpy call, ``nearest32`` of tests/nearest_reference.py, the moments added lane by lane in the stated order, Horn's matrix and the Jacobi
sweeps in Python floats (IEEE float64, each operation correctly rounded), and the loop.  Also the clouds the CPU and GPU tests share."""
import functools
import math

import numpy as np

import nearest_reference as nr

RUNNING, CONVERGED, TOO_FEW, LIMIT = range(4)
GROUP, THREADS, WAVE, QUANTITIES, SWEEPS = 1024, 256, 64, 18, 16


def transform32(points, T):
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    A = np.asarray(T, dtype=np.float64)[:3, :4].astype(np.float32)
    x, y, z = p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()
    out = np.empty_like(p)
    for r in range(3):
        s = np.add(np.multiply(A[r, 0], x), np.multiply(A[r, 1], y))
        s = np.add(s, np.multiply(A[r, 2], z))
        out[:, r] = np.add(s, A[r, 3])
    assert out.dtype == np.float32
    return out


def terms(moved, matched, dist):
    """float64 [N,18]: what one pair adds to the moments."""
    p, q, d = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (moved, matched, dist))
    t = np.zeros((len(p), QUANTITIES))
    t[:, 0] = 1.0
    for a in range(3):
        t[:, 1 + a] = p[:, a]
        t[:, 4 + a] = q[:, a]
        for b in range(3):
            t[:, 7 + 3 * a + b] = p[:, a] * q[:, b]
    t[:, 16] = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
    t[:, 17] = d * d
    return t


def butterfly(lanes):
    """[64, 18] -> [18]: v[l] += v[l ^ m] for m = 32 .. 1, every lane at once; lane 0's value."""
    v = lanes.copy()
    for m in (32, 16, 8, 4, 2, 1):
        v = np.array([v[l] + v[l ^ m] for l in range(WAVE)])
    assert all(np.array_equal(v[0], v[l]) for l in range(WAVE))
    return v[0]


def moments(moved, matched, dist, inlier):
    """float64 [18], added in the contract's order; a trimmed point is SKIPPED here (errors.py adds a zero)."""
    t = terms(moved, matched, dist)
    n = len(t)
    partials = []
    for first in range(0, n, GROUP):
        threads = np.zeros((THREADS, QUANTITIES))
        for thread in range(THREADS):
            for i in range(first + thread, min(first + GROUP, n), THREADS):
                if inlier[i]:
                    threads[thread] = threads[thread] + t[i]
        waves = [butterfly(threads[w * WAVE:(w + 1) * WAVE]) for w in range(THREADS // WAVE)]
        total = waves[0]
        for w in waves[1:]:
            total = total + w
        partials.append(total)
    lanes = np.zeros((WAVE, QUANTITIES))
    for lane in range(WAVE):
        for b in range(lane, len(partials), WAVE):
            lanes[lane] = lanes[lane] + partials[b]
    return butterfly(lanes)


def horn_matrix(S):
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = S
    return [[(Sxx + Syy) + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
            [Syz - Szy, (Sxx - Syy) - Szz, Sxy + Syx, Szx + Sxz],
            [Szx - Sxz, Sxy + Syx, (Syy - Sxx) - Szz, Syz + Szy],
            [Sxy - Syx, Szx + Sxz, Syz + Szy, (Szz - Sxx) - Syy]]


def jacobi(A):
    """Cyclic Jacobi on a symmetric 4x4 (lists of Python floats): (diagonal, V) after at most 16 sweeps."""
    A = [list(row) for row in A]
    V = [[float(r == c) for c in range(4)] for r in range(4)]
    for _ in range(SWEEPS):
        if all(A[p][q] == 0.0 for p in range(3) for q in range(p + 1, 4)):
            break
        for p in range(3):
            for q in range(p + 1, 4):
                if A[p][q] == 0.0:
                    continue
                theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q])
                t = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))
                if theta < 0.0:
                    t = -t
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for k in range(4):
                    old_p, old_q = A[k][p], A[k][q]
                    A[k][p] = c * old_p - s * old_q
                    A[k][q] = s * old_p + c * old_q
                for k in range(4):
                    old_p, old_q = A[p][k], A[q][k]
                    A[p][k] = c * old_p - s * old_q
                    A[q][k] = s * old_p + c * old_q
                A[p][q] = A[q][p] = 0.0
                for k in range(4):
                    old_p, old_q = V[k][p], V[k][q]
                    V[k][p] = c * old_p - s * old_q
                    V[k][q] = s * old_p + c * old_q
    return [A[k][k] for k in range(4)], V


def solve(m, T, with_scale=False):
    """(s R, t, T_next) from the 18 moments (n >= 3) and the current T; None where the scale's denominator is not positive."""
    m = [float(x) for x in m]
    T = [[float(x) for x in row] for row in np.asarray(T, dtype=np.float64)]
    n = m[0]
    sp, sq = m[1:4], m[4:7]
    pbar, qbar = [x / n for x in sp], [x / n for x in sq]
    S = [[m[7 + 3 * a + b] - (sp[a] * sq[b]) / n for b in range(3)] for a in range(3)]
    diagonal, V = jacobi(horn_matrix(S))
    best = max(range(4), key=lambda k: (diagonal[k], -k))                         # the largest, the lowest index on a tie
    w, x, y, z = (V[r][best] for r in range(4))
    norm = math.sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = w / norm, x / norm, y / norm, z / norm
    if w < 0.0:
        w, x, y, z = -w, -x, -y, -z
    R = [[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
         [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
         [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]]
    scale = 1.0
    if with_scale:
        denominator = m[16] - ((sp[0] * sp[0] + sp[1] * sp[1]) + sp[2] * sp[2]) / n
        if not denominator > 0.0:
            return None
        trace = 0.0
        for a in range(3):
            for b in range(3):
                trace = trace + R[a][b] * S[b][a]
        scale = trace / denominator
    M = [[scale * R[a][b] for b in range(3)] for a in range(3)]
    t = [qbar[a] - ((M[a][0] * pbar[0] + M[a][1] * pbar[1]) + M[a][2] * pbar[2]) for a in range(3)]
    rows = [[((M[a][0] * T[0][c] + M[a][1] * T[1][c]) + M[a][2] * T[2][c]) + t[a] * T[3][c] for c in range(4)] for a in range(3)]
    return np.array(M), np.array(t), np.array(rows + [T[3]])


def icp(source, target, max_distance, init=None, max_iterations=30, with_scale=False, tolerance=1e-6):
    source, target = np.asarray(source, dtype=np.float32), np.asarray(target, dtype=np.float32)
    limit = np.float32(max_distance)
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    record = {"inliers": [], "fitness": [], "rmse": [], "moments": []}
    status = RUNNING
    for k in range(max_iterations):
        moved = transform32(source, T)
        dist, index = nr.nearest32(moved, target)
        m = moments(moved, target[index], dist, dist <= limit)
        n = float(m[0])
        record["moments"].append(m)
        record["inliers"].append(int(n))
        record["fitness"].append(n / float(len(source)))
        record["rmse"].append(math.sqrt(float(m[17]) / n) if n > 0 else 0.0)
        if n < 3:
            status = TOO_FEW
            break
        if k >= 1 and abs(record["rmse"][k] - record["rmse"][k - 1]) < tolerance and abs(record["fitness"][k] - record["fitness"][k - 1]) < tolerance:
            status = CONVERGED
            break
        solved = solve(m, T, with_scale)
        if solved is None:
            status = TOO_FEW
            break
        T = solved[2]
        if k + 1 == max_iterations:
            status = LIMIT
    info = {"iterations": len(record["inliers"]), "status": status, "inliers": np.array(record["inliers"], dtype=np.int64),
            "fitness": np.array(record["fitness"]), "rmse": np.array(record["rmse"]), "moments": record["moments"][-1]}
    return T, info


# ---- shared cases ------------------------------------------------------------------------------------------------------------------------
def rotation(axis, degrees):
    axis = np.asarray(axis, dtype=np.float64)
    x, y, z = axis / np.linalg.norm(axis)
    K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    a = np.deg2rad(degrees)
    return np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)


def rigid(axis, degrees, shift, scale=1.0):
    T = np.eye(4)
    T[:3, :3] = scale * rotation(axis, degrees)
    T[:3, 3] = shift
    return T


def slanted_box(n, seed):
    """``n`` points on the six faces of a 3 x 2 m box whose top is the plane z = 1.5 + 0.9 x / 3 + 0.3 y / 2: no two faces are parallel to
    the top, the side walls have four different outlines, so the surface slides along nothing and maps onto itself only by the identity."""
    rng = np.random.default_rng(seed)
    faces = rng.integers(0, 6, n)
    u, v = rng.uniform(0.0, 1.0, n), rng.uniform(0.0, 1.0, n)

    def top(x, y):
        return 1.5 + 0.3 * x + 0.15 * y

    x = np.where(faces == 2, 0.0, np.where(faces == 3, 3.0, 3.0 * u))
    y = np.where(faces == 4, 0.0, np.where(faces == 5, 2.0, np.where(faces >= 2, 2.0 * u, 2.0 * v)))
    y = np.where((faces == 2) | (faces == 3), 2.0 * u, y)
    z = np.where(faces == 0, 0.0, np.where(faces == 1, top(x, y), v * top(x, y)))
    return np.stack([x, y, z], axis=1).astype(np.float32)


MOTION = rigid([1.0, 2.0, 3.0], 5.0, [0.02, -0.015, 0.0165])      # 5 degrees about a skew axis and 3 cm (|t| = 0.02995)


@functools.lru_cache(maxsize=None)
def box_case():
    """(source, target, motion): the 2 000-point box and its copy moved by the INVERSE of ``MOTION``, so that the registration's answer is
    ``MOTION``.  Read-only."""
    target = slanted_box(2000, 1)
    source = transform32(target, np.linalg.inv(MOTION))
    for a in (source, target):
        a.setflags(write=False)
    return source, target, MOTION


@functools.lru_cache(maxsize=None)
def box_result(with_scale=False, max_iterations=30):
    """The restatement's answer on the box (with ``with_scale``: on the source shrunk by 1.1), computed once."""
    source, target, _ = box_case()
    if with_scale:
        source = (source.astype(np.float64) / 1.1).astype(np.float32)
    return source, target, icp(source, target, 0.5, max_iterations=max_iterations, with_scale=with_scale)


def degenerate_cases():
    """(name, source, target, max_distance, the status the default loop must end with, or None where converged and limit are both fine)."""
    rng = np.random.default_rng(5)
    cloud = rng.normal(size=(300, 3)).astype(np.float32)
    plane = cloud.copy()
    plane[:, 2] = 0.25
    line = np.zeros((200, 3), np.float32)
    line[:, 0] = rng.normal(size=200)
    line[:, 1], line[:, 2] = 0.5, -1.0
    nudge = np.array([0.01, -0.02, 0.015], np.float32)
    far = cloud + np.float32(100.0)
    return [("coplanar", plane + nudge, plane, 0.5, None),
            ("collinear", line + nudge, line, 0.5, None),
            ("three", cloud[:3] + nudge, cloud, 0.5, None),
            ("two", cloud[:2] + nudge, cloud, 0.5, TOO_FEW),
            ("all_trimmed", far, cloud, 0.5, TOO_FEW),
            ("same", cloud, cloud.copy(), 0.5, CONVERGED)]

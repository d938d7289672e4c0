"""Depth-map error metrics (numpy), as reported by the reference's evaluation (/root/reference/dvmvs/errors.py:4-28)."""
import math

import numpy as np

METRIC_NAMES = ("abs_error", "abs_relative_error", "abs_inverse_error", "squared_relative_error", "rmse",
                "ratio_125", "ratio_125_2", "ratio_125_3")


def compute_errors(gt, pred, max_depth=np.inf):
    """Eight metrics over the pixels with 0.5 <= gt <= max_depth; all-NaN when no pixel qualifies."""
    keep = (gt >= 0.5) & (gt <= max_depth)
    gt, pred = gt[keep], pred[keep]
    if gt.size == 0:
        return (np.nan,) * len(METRIC_NAMES)
    n = np.float32(gt.size)
    diff = gt - pred
    ratio = np.maximum(gt / pred, pred / gt)
    thresholds = [np.count_nonzero(ratio < 1.25 ** k) / n for k in (1, 2, 3)]
    return (np.mean(np.abs(diff)),
            np.mean(np.abs(diff) / gt),
            np.mean(np.abs(1 / gt - 1 / pred)),
            np.mean(np.square(diff) / gt),
            np.sqrt(np.mean(np.square(diff))),
            *thresholds)


def compute_errors_device(gt, pred, max_depth=np.inf):
    """``compute_errors`` for depth maps that live on the GPU, as one kernel launch (dvmvs.hip.ops.depth_errors): float32 tensors
    [H,W] -> a float32 device tensor [8]; [N,H,W] or [N,1,H,W] -> [N,8].  Same per-pixel float32 terms as ``compute_errors``, summed in
    float64 on the device; nothing is copied to the host."""
    from dvmvs.hip import ops      # (imported here: this module stays importable, and compute_errors usable, without a GPU)
    rows = ops.depth_errors(gt, pred, max_depth=max_depth)
    return rows[0] if gt.dim() == 2 else rows


RECONSTRUCTION_METRICS = ("acc", "comp", "chamfer", "precision", "recall", "fscore")


def nearest_distances(query, target, return_index=False, pairs_per_chunk=1 << 22):
    """For every point of ``query`` [N,3] the distance to the nearest point of ``target`` [M,3] (M >= 1), by chunked brute force in
    float32: ``sqrt(min_j (dx*dx + dy*dy) + dz*dz)`` with ``dx = q.x - t.x`` etc., every operation an elementwise numpy operation on float32
    arrays (each rounded, nothing fused).  With ``return_index`` also the smallest index of a nearest target (int32).  This is the
    definition the device op ``dvmvs.hip.ops.nearest_distance`` reproduces bit for bit; usable on a few tens of thousands of points."""
    query = np.ascontiguousarray(query, dtype=np.float32).reshape(-1, 3)
    target = np.ascontiguousarray(target, dtype=np.float32).reshape(-1, 3)
    if len(target) == 0:
        raise ValueError("nearest_distances: the target cloud is empty")
    tx, ty, tz = (np.ascontiguousarray(target[:, a])[None, :] for a in range(3))
    dist = np.empty(len(query), dtype=np.float32)
    index = np.empty(len(query), dtype=np.int32)
    step = max(1, int(pairs_per_chunk) // len(target))
    for begin in range(0, len(query), step):
        q = query[begin:begin + step]
        dx, dy, dz = q[:, 0:1] - tx, q[:, 1:2] - ty, q[:, 2:3] - tz
        d2 = (dx * dx + dy * dy) + dz * dz
        nearest = np.argmin(d2, axis=1)                      # the first occurrence of the minimum: the smallest index
        index[begin:begin + step] = nearest
        dist[begin:begin + step] = np.sqrt(d2[np.arange(len(q)), nearest])
    return (dist, index) if return_index else dist


def reconstruction_metrics_from_distances(dist_pred, dist_gt, threshold=0.05):
    """The six metrics from the two float32 distance arrays (prediction -> ground truth, ground truth -> prediction) and the numbers of
    distances below ``threshold``: ``(float32 [6], int64 [2])``.  Means: ``math.fsum`` in float64; every entry is formed in float64 and
    rounded to float32 once."""
    if len(dist_pred) == 0 or len(dist_gt) == 0:
        raise ValueError("reconstruction metrics of an empty point cloud are undefined")
    threshold = np.float32(threshold)
    acc = math.fsum(float(d) for d in dist_pred) / len(dist_pred)
    comp = math.fsum(float(d) for d in dist_gt) / len(dist_gt)
    counts = np.array([np.count_nonzero(dist_pred < threshold), np.count_nonzero(dist_gt < threshold)], dtype=np.int64)
    precision, recall = int(counts[0]) / len(dist_pred), int(counts[1]) / len(dist_gt)
    fscore = 2.0 * precision * recall / (precision + recall) if precision + recall > 0.0 else 0.0
    return np.array([acc, comp, (acc + comp) / 2.0, precision, recall, fscore], dtype=np.float32), counts


# ----------------------------------------------------------------------------------------------------------------------
# point sets for the 3-D metrics: area-weighted samples of a triangle mesh, one point per occupied voxel
# ----------------------------------------------------------------------------------------------------------------------
SAMPLE_MAX_POINTS = 1 << 28
_AREA_SCALE = 4294967296.0          # areas are counted in units of 2^-32 square metres
_AREA_LIMIT = 1 << 63               # the total must stay below this (2^31 square metres)
VOXEL_MAX_CELLS = 1 << 21           # cells per axis of voxel_down_sample


def _lowbias32(x):
    x = np.uint32(x)
    with np.errstate(over="ignore"):
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7feb352d)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846ca68b)
        x ^= x >> np.uint32(16)
    return x


def quantised_face_areas(verts, faces):
    """``A_f = int64(rint(|e1 x e2| / 2 * 2^32))`` of every face, in float64 with every operation rounded: e1 = b - a, e2 = c - a,
    cx = e1.y e2.z - e1.z e2.y (cy, cz by the same pattern), n2 = (cx cx + cy cy) + cz cz.  A face with an index outside [0, V) has
    area 0.  Raises ``ValueError`` when an area is not finite or does not fit."""
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    valid = np.all((faces >= 0) & (faces < len(verts)), axis=1)
    safe = np.where(valid[:, None], faces, 0) if len(verts) else np.zeros_like(faces)
    if len(verts) == 0:
        return np.zeros(len(faces), dtype=np.int64), valid
    a, b, c = (verts[safe[:, j]].astype(np.float64) for j in range(3))
    e1, e2 = b - a, c - a
    with np.errstate(all="ignore"):
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        n2 = (cx * cx + cy * cy) + cz * cz
        area = np.sqrt(n2) * 0.5 * _AREA_SCALE
    area = np.where(valid, area, 0.0)
    if not np.all(area < 2.0 ** 63):       # NaN, infinite or beyond int64
        raise ValueError("sample_surface: a face's area is not finite or the mesh is larger than 2^31 square metres")
    return np.rint(area).astype(np.int64), valid


def sample_surface(verts, faces, density, seed=0, return_face=False):
    """Points on the triangle mesh ``verts`` float32 [V,3], ``faces`` int32 [F,3], about ``density`` per square metre, spread over the
    faces in proportion to their areas: float32 [N,3], with ``return_face`` also int32 [N], the face of each point.  The host definition
    that ``dvmvs.hip.ops.surface_sample`` reproduces bit for bit (include/dvmvs_hip.h restates it):
      1. ``quantised_face_areas`` and their inclusive sum ``cum`` (exact in int64; the total must stay below 2^63);
      2. D = max(int64(rint(2^32 / density)), 1); sample k sits at t_k = k D + (D >> 1) of the summed area and belongs to the face f with
         cum[f-1] <= t_k < cum[f]; N = the number of t_k below cum[F-1].  A face gets A_f / D samples to within one, a face without area
         (or with an index outside [0, V)) none;
      3. inside the face, the R2 sequence in integers: r0 = lowbias32(seed), r1 = lowbias32(seed + 1), h1 = uint32(k) 0xC13FA9A9 + r0,
         h2 = uint32(k) 0x91E10DA5 + r1, u = float32(h1 >> 8) 2^-24, v likewise; if u + v > 1 (float32): u = 1 - u, v = 1 - v;
         p = (a + u (b - a)) + v (c - a) per component in float32, every operation rounded.
    Point k depends on k and the mesh alone.  Raises ``ValueError`` for a density that is not positive and for N above 2^28."""
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    density = float(density)
    if not density > 0.0 or density == np.inf:
        raise ValueError(f"sample_surface: density must be positive and finite, got {density}")
    seed = int(seed)
    if not 0 <= seed < 2 ** 32:
        raise ValueError(f"sample_surface: seed must fit 32 unsigned bits, got {seed}")
    areas, _ = quantised_face_areas(verts, faces)
    total = (int((areas >> 32).sum()) << 32) + int((areas & 0xffffffff).sum())
    if total >= _AREA_LIMIT:
        raise ValueError("sample_surface: the mesh is larger than 2^31 square metres")
    cum = np.cumsum(areas, dtype=np.int64)
    D = max(int(np.rint(_AREA_SCALE / density)), 1)
    half = D >> 1
    N = 0 if total <= half else (total - half - 1) // D + 1
    if N > SAMPLE_MAX_POINTS:
        raise ValueError(f"sample_surface: {N} samples are more than 2^28; lower the density")
    k = np.arange(N, dtype=np.int64)
    face = np.searchsorted(cum, k * D + half, side="right").astype(np.int32)
    with np.errstate(over="ignore"):
        k32 = k.astype(np.uint32)
        h1 = k32 * np.uint32(0xC13FA9A9) + _lowbias32(seed)
        h2 = k32 * np.uint32(0x91E10DA5) + _lowbias32((seed + 1) & 0xffffffff)
    scale, one = np.float32(2.0 ** -24), np.float32(1.0)
    u = (h1 >> np.uint32(8)).astype(np.float32) * scale
    v = (h2 >> np.uint32(8)).astype(np.float32) * scale
    fold = u + v > one
    u, v = np.where(fold, one - u, u), np.where(fold, one - v, v)
    tri = faces[face]
    a, b, c = verts[tri[:, 0]], verts[tri[:, 1]], verts[tri[:, 2]]
    points = (a + u[:, None] * (b - a)) + v[:, None] * (c - a)
    return (points, face) if return_face else points


def voxel_keys(points, voxel):
    """The voxel of every point of ``voxel_down_sample``: ``(keys int64 [N], cells int32 [N,3], mn float32 [3])``."""
    points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    voxel = float(voxel)
    if len(points) == 0:
        raise ValueError("voxel_down_sample: the cloud is empty")
    if not voxel > 0.0 or voxel == np.inf:
        raise ValueError(f"voxel_down_sample: voxel must be positive and finite, got {voxel}")
    mn = points.min(axis=0)
    inv = np.float32(1.0 / voxel)
    with np.errstate(all="ignore"):
        scaled = (points - mn) * inv
    if not np.all(scaled < np.float32(VOXEL_MAX_CELLS)):
        raise ValueError("voxel_down_sample: the cloud spans 2^21 voxels or more on an axis (or holds a coordinate that is not finite)")
    cells = scaled.astype(np.int32)
    c = cells.astype(np.int64)
    return (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2], cells, mn


def voxel_down_sample(points, voxel, return_counts=False):
    """One point per occupied voxel of edge ``voxel``, the mean of the voxel's points: float32 [M,3], with ``return_counts`` also int32
    [M], the points per voxel.  ``points`` float32 [N,3], finite, N >= 1.  The host definition that ``dvmvs.hip.ops.voxel_downsample``
    reproduces bit for bit: mn = the per-axis minimum; inv = float32(1 / float64(voxel)); cell c_a = int32((x_a - mn_a) inv), a float32
    subtraction and a float32 multiplication, then truncation; key = (c_x << 42) | (c_y << 21) | c_z; the voxels come in ascending key
    order; a voxel's point is float32(sum of float64(x_i) / n) per axis, the sum in float64 over the voxel's points in ascending index i
    starting from 0.0, the division in float64.  Raises ``ValueError`` when a cell index reaches 2^21."""
    points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    keys, _, _ = voxel_keys(points, voxel)
    order = np.argsort(keys, kind="stable")
    sorted_keys = keys[order]
    starts = np.flatnonzero(np.concatenate([[True], sorted_keys[1:] != sorted_keys[:-1]]))
    counts = np.diff(np.concatenate([starts, [len(points)]]))
    sorted_points = points[order].astype(np.float64)
    # the r-th point of every voxel that has one is added in step r: each voxel's sum runs in ascending index, vectorised over the voxels
    by_count = np.argsort(-counts, kind="stable")
    descending = -counts[by_count]
    sums = np.zeros((len(starts), 3), dtype=np.float64)
    for r in range(int(counts.max())):
        active = by_count[:np.searchsorted(descending, -r, side="left")]
        sums[active] += sorted_points[starts[active] + r]
    out = (sums / counts[:, None].astype(np.float64)).astype(np.float32)
    return (out, counts.astype(np.int32)) if return_counts else out


def prepare_points(verts, faces=None, sample_density=None, voxel=None, seed=0):
    """The point set the 3-D metrics take from a surface: ``verts`` themselves, or, with ``faces`` and ``sample_density``,
    ``sample_surface(verts, faces, sample_density, seed)``; then, with ``voxel``, ``voxel_down_sample`` of that.  A side without faces (a
    point cloud) is not sampled, only down-sampled.  float32 [N,3]."""
    points = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    if sample_density is not None and faces is not None:
        points = sample_surface(points, faces, sample_density, seed)
    if voxel is not None and len(points):
        points = voxel_down_sample(points, voxel)
    return points


def prepare_points_device(verts, faces=None, sample_density=None, voxel=None, seed=0):
    """``prepare_points`` for device tensors (``dvmvs.hip.ops.surface_sample`` / ``voxel_downsample``): the same bits, on the GPU."""
    from dvmvs.hip import ops
    points = verts
    if sample_density is not None and faces is not None:
        points = ops.surface_sample(points, faces, sample_density, seed)
    if voxel is not None and points.shape[0]:
        points = ops.voxel_downsample(points, voxel)
    return points


# ----------------------------------------------------------------------------------------------------------------------
# registering the prediction to the ground truth before scoring: trimmed ICP with Horn's closed form
# ----------------------------------------------------------------------------------------------------------------------
REGISTRATION_STATUS = ("running", "converged", "too few correspondences", "iteration limit")
REGISTRATION_MAX_ITERATIONS = 1024
_ICP_BLOCK, _ICP_ROWS, _ICP_WAVE, _ICP_SWEEPS = 256, 4, 64, 16


def transform_points(points, T):
    """``points`` float32 [N,3] moved by the 4x4 ``T``: every entry of ``T[:3,:4]`` is rounded to float32 and
    ``p' = ((A00 x + A01 y) + A02 z) + A03`` (likewise y, z) is evaluated in float32, each operation rounded, nothing fused."""
    points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    A = np.asarray(T, dtype=np.float64)[:3, :4].astype(np.float32)
    x, y, z = points[:, 0].copy(), points[:, 1].copy(), points[:, 2].copy()
    return np.stack([((A[r, 0] * x + A[r, 1] * y) + A[r, 2] * z) + A[r, 3] for r in range(3)], axis=1)


def _butterfly(v):
    """The xor butterfly over axis -2 (64 entries): every entry ends as the same sum, in the order the device's wave forms it."""
    lanes = np.arange(_ICP_WAVE)
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ m, :]
    return v


def registration_moments(moved, target_points, dist, inlier):
    """The 18 float64 sums of one iteration over the inliers: n | sum p' [3] | sum q [3] | sum p' q^T [9] | sum |p'|^2 | sum d^2, added in
    the order include/dvmvs_hip.h fixes (blocks of 1024 points, 256 strided threads, wave butterfly, waves in order; then 64 strided
    lanes over the block sums and one more butterfly).  ``target_points``: q_i, the nearest target of every moved point."""
    p, q, d = moved.astype(np.float64), target_points.astype(np.float64), dist.astype(np.float64)
    n = len(p)
    terms = np.empty((n, 18), dtype=np.float64)
    terms[:, 0] = 1.0
    terms[:, 1:4], terms[:, 4:7] = p, q
    terms[:, 7:16] = (p[:, :, None] * q[:, None, :]).reshape(n, 9)
    terms[:, 16] = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
    terms[:, 17] = d * d
    terms[~inlier] = 0.0                                       # a skipped point and an added +0.0 are the same bits
    group = _ICP_BLOCK * _ICP_ROWS
    groups = -(-n // group)
    padded = np.zeros((groups * group, 18), dtype=np.float64)
    padded[:n] = terms
    padded = padded.reshape(groups, _ICP_ROWS, _ICP_BLOCK, 18)
    threads = np.zeros((groups, _ICP_BLOCK, 18), dtype=np.float64)
    for r in range(_ICP_ROWS):
        threads = threads + padded[:, r]
    waves = _butterfly(threads.reshape(groups, _ICP_BLOCK // _ICP_WAVE, _ICP_WAVE, 18))[:, :, 0]
    partials = waves[:, 0]
    for w in range(1, _ICP_BLOCK // _ICP_WAVE):
        partials = partials + waves[:, w]
    rounds = -(-groups // _ICP_WAVE)
    padded = np.zeros((rounds * _ICP_WAVE, 18), dtype=np.float64)
    padded[:groups] = partials
    padded = padded.reshape(rounds, _ICP_WAVE, 18)
    lanes = np.zeros((_ICP_WAVE, 18), dtype=np.float64)
    for r in range(rounds):
        lanes = lanes + padded[r]
    return _butterfly(lanes)[0]


def _horn_quaternion(S):
    """(w, x, y, z), w >= 0: the eigenvector of the largest eigenvalue of Horn's symmetric 4x4 matrix of ``S`` (nine floats, row-major),
    by cyclic Jacobi sweeps in float64 with +, -, *, / and sqrt only (Python floats: each operation correctly rounded)."""
    Sxx, Sxy, Sxz, Syx, Syy, Syz, Szx, Szy, Szz = S
    A = [[(Sxx + Syy) + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
         [Syz - Szy, (Sxx - Syy) - Szz, Sxy + Syx, Szx + Sxz],
         [Szx - Sxz, Sxy + Syx, (Syy - Sxx) - Szz, Syz + Szy],
         [Sxy - Syx, Szx + Sxz, Syz + Szy, (Szz - Sxx) - Syy]]
    V = [[1.0 if r == c else 0.0 for c in range(4)] for r in range(4)]
    pairs = [(p, q) for p in range(3) for q in range(p + 1, 4)]
    for _ in range(_ICP_SWEEPS):
        if all(A[p][q] == 0.0 for p, q in pairs):
            break
        for p, q in pairs:
            apq = A[p][q]
            if apq == 0.0:
                continue
            theta = (A[q][q] - A[p][p]) / (2.0 * apq)
            mag = abs(theta) + math.sqrt(theta * theta + 1.0)
            t = -1.0 / mag if theta < 0.0 else 1.0 / mag
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            for k in range(4):
                akp, akq = A[k][p], A[k][q]
                A[k][p], A[k][q] = c * akp - s * akq, s * akp + c * akq
            for k in range(4):
                apk, aqk = A[p][k], A[q][k]
                A[p][k], A[q][k] = c * apk - s * aqk, s * apk + c * aqk
            A[p][q] = A[q][p] = 0.0
            for k in range(4):
                vkp, vkq = V[k][p], V[k][q]
                V[k][p], V[k][q] = c * vkp - s * vkq, s * vkp + c * vkq
    best = 0
    for k in range(1, 4):
        if A[k][k] > A[best][best]:
            best = k
    w, x, y, z = (V[r][best] for r in range(4))
    norm = math.sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = w / norm, x / norm, y / norm, z / norm
    return (-w, -x, -y, -z) if w < 0.0 else (w, x, y, z)


def registration_solve(moments, T, with_scale=False):
    """The update of one iteration from its 18 sums (n >= 3): the float64 4x4 ``[sR t; 0 1] T``, or None where the scale's denominator is
    not positive.  Every operation in float64, in the order include/dvmvs_hip.h states."""
    v = [float(m) for m in moments]
    with np.errstate(all="ignore"):
        return _registration_solve(v, [[float(e) for e in row] for row in np.asarray(T, dtype=np.float64)], with_scale)


def _registration_solve(v, T, with_scale):
    n = v[0]
    pbar, qbar = [v[1 + a] / n for a in range(3)], [v[4 + a] / n for a in range(3)]
    S = [v[7 + a * 3 + b] - (v[1 + a] * v[4 + b]) / n for a in range(3) for b in range(3)]
    w, x, y, z = _horn_quaternion(S)
    R = [1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
         2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
         2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]
    scale = 1.0
    if with_scale:
        denominator = v[16] - ((v[1] * v[1] + v[2] * v[2]) + v[3] * v[3]) / n
        if not denominator > 0.0:
            return None
        trace = 0.0
        for a in range(3):
            for b in range(3):
                trace += R[a * 3 + b] * S[b * 3 + a]
        scale = trace / denominator
    M = [scale * r for r in R]
    shift = [qbar[a] - ((M[a * 3] * pbar[0] + M[a * 3 + 1] * pbar[1]) + M[a * 3 + 2] * pbar[2]) for a in range(3)]
    out = [[((M[a * 3] * T[0][c] + M[a * 3 + 1] * T[1][c]) + M[a * 3 + 2] * T[2][c]) + shift[a] * T[3][c] for c in range(4)] for a in range(3)]
    return np.array(out + [T[3]], dtype=np.float64)


def register_points(source, target, max_distance, init=None, max_iterations=30, with_scale=False, tolerance=1e-6):
    """Registers ``source`` [N,3] to ``target`` [M,3] by trimmed ICP: ``(T float64 [4,4], info)``, ``T`` taking source coordinates into the
    target's frame.  The host definition that ``dvmvs.hip.registration.icp`` reproduces bit for bit (include/dvmvs_hip.h restates it).
    Iteration k, from ``T_0 = init`` (or the identity): the source moved by ``transform_points``; its nearest targets by
    ``nearest_distances`` (float32, smallest index); the inliers ``d <= float32(max_distance)``; their ``registration_moments``;
    rmse_k = sqrt(sum d^2 / n) (0 without inliers) and fitness_k = n / N, which describe T_k; fewer than 3 inliers stop with status 2;
    from k = 1 on, rmse and fitness both within ``tolerance`` (strictly) of the iteration before stop with status 1 and leave T; otherwise
    ``registration_solve`` (Horn's quaternion by Jacobi sweeps, Umeyama's scale with ``with_scale``) gives T_{k+1}; status 3 at the limit.
    ``info``: ``iterations``, ``status`` (an index of ``REGISTRATION_STATUS``), and per recorded iteration ``inliers`` (int64), ``fitness``,
    ``rmse`` (float64), with ``moments``, the sums of the last one."""
    source = np.ascontiguousarray(source, dtype=np.float32).reshape(-1, 3)
    target = np.ascontiguousarray(target, dtype=np.float32).reshape(-1, 3)
    max_distance, tolerance, max_iterations = np.float32(max_distance), float(tolerance), int(max_iterations)
    if len(source) == 0 or len(target) == 0:
        raise ValueError("register_points: both point clouds must hold at least one point")
    if not max_distance > 0.0 or not tolerance >= 0.0:
        raise ValueError(f"register_points: max_distance must be positive and tolerance not negative, got {max_distance}, {tolerance}")
    if not 1 <= max_iterations <= REGISTRATION_MAX_ITERATIONS:
        raise ValueError(f"register_points: max_iterations must be in 1 .. {REGISTRATION_MAX_ITERATIONS}, got {max_iterations}")
    T = np.eye(4, dtype=np.float64) if init is None else np.array(init, dtype=np.float64)
    if T.shape != (4, 4) or not np.isfinite(T).all():
        raise ValueError("register_points: init must be a finite 4x4 matrix")
    inliers, fitness, rmse = [], [], []
    status, moments = 0, np.zeros(18, dtype=np.float64)
    for k in range(max_iterations):
        moved = transform_points(source, T)
        dist, index = nearest_distances(moved, target, return_index=True)
        moments = registration_moments(moved, target[index], dist, dist <= max_distance)
        n = float(moments[0])
        inliers.append(int(n))
        fitness.append(n / float(len(source)))
        rmse.append(math.sqrt(float(moments[17]) / n) if n > 0.0 else 0.0)
        if n < 3.0:
            status = 2
            break
        if k >= 1 and abs(rmse[k] - rmse[k - 1]) < tolerance and abs(fitness[k] - fitness[k - 1]) < tolerance:
            status = 1
            break
        update = registration_solve(moments, T, with_scale)
        if update is None:
            status = 2
            break
        T = update
        if k + 1 == max_iterations:
            status = 3
    info = {"iterations": len(inliers), "status": status, "inliers": np.array(inliers, dtype=np.int64),
            "fitness": np.array(fitness, dtype=np.float64), "rmse": np.array(rmse, dtype=np.float64), "moments": moments}
    return T, info


def register_points_device(source, target, max_distance, init=None, max_iterations=30, with_scale=False, tolerance=1e-6, grid=None):
    """``register_points`` for device tensors (``dvmvs.hip.registration.icp``): the same bits, ``T`` and every entry of ``info`` on the GPU,
    nothing read by the call.  ``grid``: an existing ``ops.nearest_build`` workspace of ``target``."""
    from dvmvs.hip import registration
    return registration.icp(source, target, max_distance, init=init, max_iterations=max_iterations, with_scale=with_scale, tolerance=tolerance,
                            grid=grid)


# ----------------------------------------------------------------------------------------------------------------------
# point-to-plane registration: the same loop with the target's normals, a 6x6 linearised step instead of Horn's closed form
# ----------------------------------------------------------------------------------------------------------------------
REGISTRATION_PLANE_STATUS = ("running", "converged", "too few correspondences", "iteration limit", "degenerate geometry")
REGISTRATION_PLANE_MOMENTS = 30
REGISTRATION_PLANE_MIN_INLIERS = 6
REGISTRATION_PLANE_PIVOT = 2.0 ** -30           # a pivot of the LDL^T must exceed this share of its diagonal entry


def has_normal(normals):
    """bool [M]: the rows of ``normals`` float32 [M,3] that are finite and not all zero."""
    normals = np.asarray(normals, dtype=np.float32).reshape(-1, 3)
    return np.isfinite(normals).all(axis=1) & (normals != 0.0).any(axis=1)


def _ordered_sums(terms):
    """The column sums of ``terms`` float64 [N,C] in the order of ``registration_moments``: blocks of 1024 rows, 256 strided threads x 4
    rows, wave butterfly, waves in order; then 64 strided lanes over the block sums and one more butterfly."""
    n, columns = terms.shape
    group = _ICP_BLOCK * _ICP_ROWS
    groups = -(-n // group)
    padded = np.zeros((groups * group, columns), dtype=np.float64)
    padded[:n] = terms
    padded = padded.reshape(groups, _ICP_ROWS, _ICP_BLOCK, columns)
    threads = np.zeros((groups, _ICP_BLOCK, columns), dtype=np.float64)
    for r in range(_ICP_ROWS):
        threads = threads + padded[:, r]
    waves = _butterfly(threads.reshape(groups, _ICP_BLOCK // _ICP_WAVE, _ICP_WAVE, columns))[:, :, 0]
    partials = waves[:, 0]
    for w in range(1, _ICP_BLOCK // _ICP_WAVE):
        partials = partials + waves[:, w]
    rounds = -(-groups // _ICP_WAVE)
    padded = np.zeros((rounds * _ICP_WAVE, columns), dtype=np.float64)
    padded[:groups] = partials
    padded = padded.reshape(rounds, _ICP_WAVE, columns)
    lanes = np.zeros((_ICP_WAVE, columns), dtype=np.float64)
    for r in range(rounds):
        lanes = lanes + padded[r]
    return _butterfly(lanes)[0]


def registration_plane_moments(moved, target_points, target_normals, dist, inlier):
    """The 30 float64 sums of one point-to-plane iteration over the inliers: n | sum J_a J_b for a <= b, row-major [21] | sum J_a r [6] |
    sum r^2 | sum d^2, with p = moved_i, q, n = the nearest target and its normal, o = moved_0 (inlier or not),
    r = ((p0-q0) n0 + (p1-q1) n1) + (p2-q2) n2, c = (p - o) x n, J = (c0, c1, c2, n0, n1, n2); every product and sum rounded to float64,
    nothing fused; added in the order of ``registration_moments``.  ``target_points``, ``target_normals``: q_i and n_i per moved point."""
    p, q, nn, d = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (moved, target_points, target_normals, dist))
    inlier = np.asarray(inlier, dtype=bool)
    n = len(p)
    terms = np.empty((n, REGISTRATION_PLANE_MOMENTS), dtype=np.float64)
    with np.errstate(all="ignore"):
        e = p - p[0]
        r = ((p[:, 0] - q[:, 0]) * nn[:, 0] + (p[:, 1] - q[:, 1]) * nn[:, 1]) + (p[:, 2] - q[:, 2]) * nn[:, 2]
        J = np.stack([e[:, 1] * nn[:, 2] - e[:, 2] * nn[:, 1], e[:, 2] * nn[:, 0] - e[:, 0] * nn[:, 2], e[:, 0] * nn[:, 1] - e[:, 1] * nn[:, 0],
                      nn[:, 0], nn[:, 1], nn[:, 2]], axis=1)
        terms[:, 0] = 1.0
        column = 1
        for a in range(6):
            for b in range(a, 6):
                terms[:, column] = J[:, a] * J[:, b]
                column += 1
        for a in range(6):
            terms[:, 22 + a] = J[:, a] * r
        terms[:, 28] = r * r
        terms[:, 29] = d * d
    terms[~inlier] = 0.0                                       # a skipped point and an added +0.0 are the same bits
    return _ordered_sums(terms)


def _registration_plane_moments_loop(moved, target_points, target_normals, dist, inlier):
    """``registration_plane_moments`` point by point in Python floats, as a thread of the device adds them: a trimmed point is skipped."""
    rows = [np.asarray(a, dtype=np.float32).astype(np.float64).tolist() for a in (moved, target_points, target_normals)]
    d = np.asarray(dist, dtype=np.float32).astype(np.float64).tolist()
    count, C = len(d), REGISTRATION_PLANE_MOMENTS
    o = rows[0][0]

    def butterfly(lanes):
        for m in (32, 16, 8, 4, 2, 1):
            lanes = [[lanes[l][k] + lanes[l ^ m][k] for k in range(C)] for l in range(_ICP_WAVE)]
        return lanes[0]

    group = _ICP_BLOCK * _ICP_ROWS
    partials = []
    for first in range(0, count, group):
        threads = [[0.0] * C for _ in range(_ICP_BLOCK)]
        for t in range(_ICP_BLOCK):
            v = threads[t]
            for i in range(first + t, min(first + group, count), _ICP_BLOCK):
                if not inlier[i]:
                    continue
                p, q, n = rows[0][i], rows[1][i], rows[2][i]
                e = [p[0] - o[0], p[1] - o[1], p[2] - o[2]]
                r = ((p[0] - q[0]) * n[0] + (p[1] - q[1]) * n[1]) + (p[2] - q[2]) * n[2]
                J = [e[1] * n[2] - e[2] * n[1], e[2] * n[0] - e[0] * n[2], e[0] * n[1] - e[1] * n[0], n[0], n[1], n[2]]
                v[0] += 1.0
                column = 1
                for a in range(6):
                    for b in range(a, 6):
                        v[column] += J[a] * J[b]
                        column += 1
                for a in range(6):
                    v[22 + a] += J[a] * r
                v[28] += r * r
                v[29] += d[i] * d[i]
        waves = [butterfly(threads[w * _ICP_WAVE:(w + 1) * _ICP_WAVE]) for w in range(_ICP_BLOCK // _ICP_WAVE)]
        total = waves[0]
        for w in waves[1:]:
            total = [a + b for a, b in zip(total, w)]
        partials.append(total)
    lanes = [[0.0] * C for _ in range(_ICP_WAVE)]
    for lane in range(_ICP_WAVE):
        for b in range(lane, len(partials), _ICP_WAVE):
            lanes[lane] = [x + y for x, y in zip(lanes[lane], partials[b])]
    return np.array(butterfly(lanes), dtype=np.float64)


def _ldlt_solve(A, b):
    """x with A x = -b for a symmetric 6x6 ``A`` (lists of Python floats; the lower triangle is read), by LDL^T without pivoting in the
    order include/dvmvs_hip.h states; None when a pivot is not above ``REGISTRATION_PLANE_PIVOT`` times its diagonal entry."""
    L = [[0.0] * 6 for _ in range(6)]
    D = [0.0] * 6
    for j in range(6):
        d = A[j][j]
        for k in range(j):
            d = d - (L[j][k] * L[j][k]) * D[k]
        if not d > REGISTRATION_PLANE_PIVOT * A[j][j]:
            return None
        D[j] = d
        for i in range(j + 1, 6):
            s = A[i][j]
            for k in range(j):
                s = s - (L[i][k] * L[j][k]) * D[k]
            L[i][j] = s / d
    x = [0.0] * 6
    for i in range(6):
        s = -b[i]
        for k in range(i):
            s = s - L[i][k] * x[k]
        x[i] = s
    for i in range(6):
        x[i] = x[i] / D[i]
    for i in range(5, -1, -1):
        s = x[i]
        for k in range(i + 1, 6):
            s = s - L[k][i] * x[k]
        x[i] = s
    return x


def _plane_system(v):
    A = [[0.0] * 6 for _ in range(6)]
    column = 1
    for a in range(6):
        for b in range(a, 6):
            A[a][b] = A[b][a] = v[column]
            column += 1
    return A, v[22:28]


def registration_plane_solve(moments, T, origin):
    """The update of one point-to-plane iteration from its 30 sums: the float64 4x4 ``[R, (o - R o) + t; 0 1] T`` with ``origin`` = o (the
    first moved point), or None for degenerate geometry (a pivot of the LDL^T at or below 2^-30 of its diagonal entry).  x = (alpha, beta,
    gamma, t) solves (sum J J^T) x = -(sum J r); the rotation is that of the unit quaternion (1, alpha/2, beta/2, gamma/2) / norm.  Every
    operation in float64, in the order include/dvmvs_hip.h states."""
    v = [float(m) for m in moments]
    T = [[float(e) for e in row] for row in np.asarray(T, dtype=np.float64)]
    o = [float(e) for e in np.asarray(origin, dtype=np.float32)]
    with np.errstate(all="ignore"):
        A, b = _plane_system(v)
        step = _ldlt_solve(A, b)
        if step is None:
            return None
        x, y, z = step[0] / 2.0, step[1] / 2.0, step[2] / 2.0
        norm = math.sqrt(((1.0 + x * x) + y * y) + z * z)
        w, x, y, z = 1.0 / norm, x / norm, y / norm, z / norm
        R = [1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
             2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
             2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]
        shift = [(o[a] - ((R[a * 3] * o[0] + R[a * 3 + 1] * o[1]) + R[a * 3 + 2] * o[2])) + step[3 + a] for a in range(3)]
        out = [[((R[a * 3] * T[0][c] + R[a * 3 + 1] * T[1][c]) + R[a * 3 + 2] * T[2][c]) + shift[a] * T[3][c] for c in range(4)]
               for a in range(3)]
    return np.array(out + [T[3]], dtype=np.float64)


def register_points_plane(source, target, target_normals, max_distance, init=None, max_iterations=30, tolerance=1e-6):
    """Registers ``source`` [N,3] to ``target`` [M,3] with normals ``target_normals`` float32 [M,3] by trimmed point-to-plane ICP:
    ``(T float64 [4,4], info)``.  The host definition that ``dvmvs.hip.registration.icp_plane`` reproduces bit for bit (include/dvmvs_hip.h
    restates it).  A normal that is all zero or not finite is "no normal"; a normal's sign does not matter (every term is even in it).
    Iteration k, from ``T_0 = init`` (or the identity): the source moved by ``transform_points``; its nearest targets by
    ``nearest_distances``; the inliers ``d <= float32(max_distance)`` whose target has a normal; their ``registration_plane_moments``;
    rmse_k = sqrt(sum r^2 / n) (the plane residual; 0 without inliers), rmse_point_k = sqrt(sum d^2 / n) and fitness_k = n / N, which
    describe T_k; fewer than 6 inliers stop with status 2; from k = 1 on, rmse and fitness both within ``tolerance`` (strictly) of the
    iteration before stop with status 1 and leave T; otherwise ``registration_plane_solve`` gives T_{k+1}, or stops with status 4 and leaves
    T where the geometry does not fix all six freedoms; status 3 at the limit.  ``info``: ``iterations``, ``status`` (an index of
    ``REGISTRATION_PLANE_STATUS``), and per recorded iteration ``inliers`` (int64), ``fitness``, ``rmse``, ``rmse_point`` (float64), with
    ``moments`` [30], the sums of the last one."""
    source = np.ascontiguousarray(source, dtype=np.float32).reshape(-1, 3)
    target = np.ascontiguousarray(target, dtype=np.float32).reshape(-1, 3)
    target_normals = np.ascontiguousarray(target_normals, dtype=np.float32)
    max_distance, tolerance, max_iterations = np.float32(max_distance), float(tolerance), int(max_iterations)
    if len(source) == 0 or len(target) == 0:
        raise ValueError("register_points_plane: both point clouds must hold at least one point")
    if target_normals.shape != target.shape:
        raise ValueError(f"register_points_plane: target_normals must be float32 {target.shape} like the target, got {target_normals.shape}")
    if not max_distance > 0.0 or not tolerance >= 0.0:
        raise ValueError(f"register_points_plane: max_distance must be positive and tolerance not negative, got {max_distance}, {tolerance}")
    if not 1 <= max_iterations <= REGISTRATION_MAX_ITERATIONS:
        raise ValueError(f"register_points_plane: max_iterations must be in 1 .. {REGISTRATION_MAX_ITERATIONS}, got {max_iterations}")
    T = np.eye(4, dtype=np.float64) if init is None else np.array(init, dtype=np.float64)
    if T.shape != (4, 4) or not np.isfinite(T).all():
        raise ValueError("register_points_plane: init must be a finite 4x4 matrix")
    with_normal = has_normal(target_normals)
    inliers, fitness, rmse, rmse_point = [], [], [], []
    status, moments = 0, np.zeros(REGISTRATION_PLANE_MOMENTS, dtype=np.float64)
    for k in range(max_iterations):
        moved = transform_points(source, T)
        dist, index = nearest_distances(moved, target, return_index=True)
        moments = registration_plane_moments(moved, target[index], target_normals[index], dist, (dist <= max_distance) & with_normal[index])
        n = float(moments[0])
        inliers.append(int(n))
        fitness.append(n / float(len(source)))
        rmse.append(math.sqrt(float(moments[28]) / n) if n > 0.0 else 0.0)
        rmse_point.append(math.sqrt(float(moments[29]) / n) if n > 0.0 else 0.0)
        if n < float(REGISTRATION_PLANE_MIN_INLIERS):
            status = 2
            break
        if k >= 1 and abs(rmse[k] - rmse[k - 1]) < tolerance and abs(fitness[k] - fitness[k - 1]) < tolerance:
            status = 1
            break
        update = registration_plane_solve(moments, T, moved[0])
        if update is None:
            status = 4
            break
        T = update
        if k + 1 == max_iterations:
            status = 3
    info = {"iterations": len(inliers), "status": status, "inliers": np.array(inliers, dtype=np.int64),
            "fitness": np.array(fitness, dtype=np.float64), "rmse": np.array(rmse, dtype=np.float64),
            "rmse_point": np.array(rmse_point, dtype=np.float64), "moments": moments}
    return T, info


def register_points_plane_device(source, target, target_normals, max_distance, init=None, max_iterations=30, tolerance=1e-6, grid=None):
    """``register_points_plane`` for device tensors (``dvmvs.hip.registration.icp_plane``): the same bits, ``T`` and every entry of ``info``
    on the GPU, nothing read by the call.  ``grid``: an existing ``ops.nearest_build`` workspace of ``target``."""
    from dvmvs.hip import registration
    return registration.icp_plane(source, target, target_normals, max_distance, init=init, max_iterations=max_iterations, tolerance=tolerance,
                                  grid=grid)


def _check_alignment(name, align_distance, align_scale, align_init, return_transform):
    if align_distance is None and (align_scale or align_init is not None or return_transform):
        raise ValueError(f"{name}: align_scale, align_init and return_transform say how align_distance registers: they need align_distance")


def _check_plane(name, align_plane, align_distance, align_scale, gt_normals, gt_replaced, neighbours, normal_distance):
    """The point-to-plane keywords of the scoring functions: ``align_plane`` needs ``align_distance`` and excludes ``align_scale``; the
    other three say how it registers."""
    if not isinstance(align_plane, (bool, np.bool_)):
        raise ValueError(f"{name}: align_plane must be a bool, got {align_plane!r}")
    if not align_plane:
        if gt_normals is not None or neighbours != 20 or normal_distance != np.inf:
            raise ValueError(f"{name}: gt_normals, align_normal_neighbours and align_normal_distance say how align_plane registers: they need "
                             f"align_plane")
        return
    if align_distance is None:
        raise ValueError(f"{name}: align_plane says how align_distance registers: it needs align_distance")
    if align_scale:
        raise ValueError(f"{name}: align_plane finds a rigid motion; it excludes align_scale")
    if gt_normals is not None and gt_replaced:
        raise ValueError(f"{name}: gt_normals are the normals of gt_points as given; face sampling and voxel down-sampling replace those "
                         f"points (leave gt_normals out: the normals are then estimated)")


def compute_reconstruction_errors(pred_points, gt_points, threshold=0.05, pred_faces=None, gt_faces=None, sample_density=None, voxel=None,
                                  align_plane=False, gt_normals=None, align_normal_neighbours=20, align_normal_distance=np.inf,
                                  align_distance=None, align_scale=False, align_init=None, return_transform=False):
    """The 3-D reconstruction metrics of the Atlas / NeuralRecon / SimpleRecon evaluations between a predicted point set [N,3] and a
    ground-truth point set [M,3], float32 [6] in the order of ``RECONSTRUCTION_METRICS``:
      acc = mean distance from a predicted point to its nearest ground-truth point; comp = the same from ground truth to prediction;
      chamfer = (acc + comp) / 2; precision = share of predicted points closer than ``threshold`` (strictly) to the ground truth;
      recall = share of ground-truth points closer than ``threshold`` to the prediction; fscore = 2PR / (P + R), 0 when P + R = 0.
    The host definition: numpy, exact nearest neighbours by chunked brute force (``nearest_distances``), for a few tens of thousands of
    points.  The distances are point-to-point.  With every keyword at None the point sets are taken as they come; in this package they
    are then MESH VERTICES (``TSDFVolume.score_against``), one per crossed grid edge, which compares two marching-cubes meshes of one
    voxel size soundly and nothing else.  The usual protocol is the keywords: ``pred_faces`` / ``gt_faces`` (int32 [F,3]) with
    ``sample_density`` (points per square metre) replace a side's vertices by ``sample_surface`` of its mesh, and ``voxel`` (metres)
    replaces each side by its ``voxel_down_sample``, so that both clouds have a common resolution (``prepare_points``).  Raises
    ``ValueError`` when either set is, or becomes, empty.

    ``align_distance`` (metres): the prediction's prepared point set is first registered to the ground truth's by ``register_points`` with
    that inlier distance (``align_scale``: a similarity instead of a rigid motion; ``align_init``: a 4x4 to start from), moved by the
    result (``transform_points``) and then scored, as the Tanks-and-Temples evaluation does; ``return_transform``: return
    ``(row, T float64 [4,4])``.  With ``align_distance`` at None nothing is registered and the row is what it is without the keywords.

    ``align_plane`` (needs ``align_distance``, excludes ``align_scale``): the registration is ``register_points_plane``, point-to-plane
    on the ground truth's normals, which does not crawl along walls and floors as point-to-point does.  ``gt_normals`` float32 [M,3]: the
    normals of ``gt_points`` as given (an error together with ``gt_faces`` sampling or ``voxel``, which replace the points); without
    them the normals are ``dvmvs.normals.estimate_normals`` of the prepared ground-truth points from ``align_normal_neighbours`` nearest
    points within ``align_normal_distance``."""
    _check_alignment("compute_reconstruction_errors", align_distance, align_scale, align_init, return_transform)
    _check_plane("compute_reconstruction_errors", align_plane, align_distance, align_scale, gt_normals,
                 (gt_faces is not None and sample_density is not None) or voxel is not None, align_normal_neighbours, align_normal_distance)
    pred_points = prepare_points(pred_points, pred_faces, sample_density, voxel)
    gt_points = prepare_points(gt_points, gt_faces, sample_density, voxel)
    if len(pred_points) == 0 or len(gt_points) == 0:
        raise ValueError("compute_reconstruction_errors: both point clouds must hold at least one point")
    transform = None
    if align_plane:
        if gt_normals is None:
            from dvmvs.normals import estimate_normals
            gt_normals = estimate_normals(gt_points, align_normal_neighbours, align_normal_distance)[0]
        transform, _ = register_points_plane(pred_points, gt_points, gt_normals, align_distance, init=align_init)
        pred_points = transform_points(pred_points, transform)
    elif align_distance is not None:
        transform, _ = register_points(pred_points, gt_points, align_distance, init=align_init, with_scale=align_scale)
        pred_points = transform_points(pred_points, transform)
    row = reconstruction_metrics_from_distances(nearest_distances(pred_points, gt_points), nearest_distances(gt_points, pred_points),
                                                threshold)[0]
    return (row, transform) if return_transform else row


def compute_reconstruction_errors_device(pred_points, gt_points, threshold=0.05, counts=None, pred_faces=None, gt_faces=None,
                                         sample_density=None, voxel=None, align_plane=False, gt_normals=None, align_normal_neighbours=20,
                                         align_normal_distance=np.inf, align_distance=None, align_scale=False, align_init=None,
                                         return_transform=False):
    """``compute_reconstruction_errors`` for point sets that live on the GPU (float32 [N,3] and [M,3] device tensors, both non-empty):
    a float32 device tensor [6].  Two grid builds, two nearest-point queries (csrc/nearest_points.hip: the distances are the host
    function's, bit for bit) and one reduction in float64, all on the current stream; with every keyword at None nothing is copied to
    the host.  ``counts``: an int64 [2] device tensor that receives the numbers of distances below the threshold.  ``pred_faces`` /
    ``gt_faces`` (int32 [F,3] device tensors), ``sample_density`` and ``voxel`` as in the host function, on the device
    (csrc/surface_sample.hip: the host definitions' bits; each sampling and each down-sampling reads its output's size once).
    ``align_distance``, ``align_scale``, ``align_init`` (a HOST 4x4) and ``return_transform`` as in the host function: the registration
    (``dvmvs.hip.registration.icp``: the host definition's bits, no host read) uses the ground truth's grid, which then also serves the
    accuracy query; the transform comes back as a float64 [4,4] device tensor.  ``align_plane``, ``gt_normals`` (a float32 [M,3] device
    tensor), ``align_normal_neighbours`` and ``align_normal_distance`` as in the host function (``dvmvs.hip.registration.icp_plane``);
    normals that are not given are estimated on the same grid (``dvmvs.hip.normals.estimate_normals``)."""
    _check_alignment("compute_reconstruction_errors_device", align_distance, align_scale, align_init, return_transform)
    _check_plane("compute_reconstruction_errors_device", align_plane, align_distance, align_scale, gt_normals,
                 (gt_faces is not None and sample_density is not None) or voxel is not None, align_normal_neighbours, align_normal_distance)
    row, transform, _ = _score_device(pred_points, gt_points, threshold, counts, pred_faces, gt_faces, sample_density, voxel, align_distance,
                                      align_scale, align_init, align_plane, gt_normals, align_normal_neighbours, align_normal_distance)
    return (row, transform) if return_transform else row


def _score_device(pred_points, gt_points, threshold, counts, pred_faces, gt_faces, sample_density, voxel, align_distance, align_scale,
                  align_init, align_plane=False, gt_normals=None, align_normal_neighbours=20, align_normal_distance=np.inf):
    """``compute_reconstruction_errors_device``: ``(row, transform or None, the registration's info or None)``."""
    from dvmvs.hip import ops      # (imported here: this module stays importable, and the host functions usable, without a GPU)
    transform = info = None
    if pred_faces is not None or gt_faces is not None or sample_density is not None or voxel is not None:
        pred_points = prepare_points_device(pred_points, pred_faces, sample_density, voxel)
        gt_points = prepare_points_device(gt_points, gt_faces, sample_density, voxel)
    for label, t in (("pred_points", pred_points), ("gt_points", gt_points)):
        if hasattr(t, "shape") and len(t.shape) == 2 and t.shape[0] == 0:
            raise ValueError(f"compute_reconstruction_errors_device: {label} is empty")
    if align_distance is None:
        dist_pred = ops.nearest_distance(pred_points, gt_points)
    else:       # one grid of the ground truth serves the registration's queries and the accuracy query
        from dvmvs.hip import registration
        grid = ops.nearest_build(gt_points)
        if align_plane:
            if gt_normals is None:
                from dvmvs.hip import normals
                gt_normals = normals.estimate_normals(gt_points, align_normal_neighbours, align_normal_distance, grid=grid)[0]
            transform, info = registration.icp_plane(pred_points, gt_points, gt_normals, align_distance, init=align_init, grid=grid)
        else:
            transform, info = registration.icp(pred_points, gt_points, align_distance, init=align_init, with_scale=align_scale, grid=grid)
        pred_points = registration.transform_points(pred_points, transform)
        dist_pred = ops.nearest_query(pred_points, gt_points, grid)
    dist_gt = ops.nearest_distance(gt_points, pred_points)
    return ops.distance_metrics(dist_pred, dist_gt, threshold, counts=counts), transform, info

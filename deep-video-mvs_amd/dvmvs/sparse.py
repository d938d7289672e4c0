"""Host definition of the sparse TSDF volume's MARKING: which 8 x 8 x 8-voxel bricks a depth frame allocates.
Plain numpy in float32, no device; ``mark_bricks`` is the definition and the mark kernel of csrc/sparse_volume.hip reproduces it bit for
bit (contraction off there; every operation below is one IEEE float32 operation, in the order the parentheses give).

Voxel ``v`` (a signed integer triple) lies at ``origin + float(v) * voxel_size``; brick ``b = floor(v / 8)``, ``|b| < 2^20``.

The rule, per pixel (u, v) with depth d after ``d > max_depth -> 0``; f32 throughout:
  * ``d`` that is not > 0 or not finite marks nothing.
  * ``z0 = max(d - trunc, 0)``, ``z1 = d + trunc``, ``k = clamp(ceil((z1 - z0) / (2 s)), 1, 16)`` intervals, ``delta = (z1 - z0) / k``.
  * ``a = (u - cx) / fx``, ``b = (v - cy) / fy``; ``r_pix = sqrt((1/fx)(1/fx) + (1/fy)(1/fy))``, ``r_ray = sqrt((1 + a a) + b b)``.
  * ``W = ((|o0| + |o1|) + |o2|) + ((|t0| + |t1|) + |t2|) + z1 ((1 + |a|) + |b|)`` and ``slack = 1e-4 s + 2^-18 W``.
  * samples ``z_i = z0 + float(i) delta``, i = 0 .. k: margin ``m_i = ((HALF (z_i + delta / 2)) r_pix + (delta / 2) r_ray) + slack`` with
    ``HALF = 0.501953125`` (half a pixel, times 1 + 2^-8 for the rounding of the projection), and the world point
    ``S_c = ((R[c][0] (a z_i) + R[c][1] (b z_i)) + R[c][2] z_i) + t_c`` of the camera-to-world pose.
  * the sample's bricks, per axis c: ``floor(((S_c - m_i) - o_c) / (8 s)) .. floor(((S_c + m_i) - o_c) / (8 s))``.
  * a pixel with ANY sample whose range leaves ``|b| < 2^20``, is not finite, or spans more than 4 bricks on an axis marks NOTHING and is
    counted as rejected (a footprint of more than 32 voxels says the voxel size does not suit the frame).
"""
import numpy as np

BRICK = 8
BRICK_LIMIT = (1 << 20) - 1
MAX_INTERVALS = 16
MAX_SPAN = 4
HALF_PIXEL = np.float32(0.501953125)
SLACK_VOXELS = np.float32(1e-4)
SLACK_RELATIVE = np.float32(2.0 ** -18)
_F32_MAX = np.float32(3.4028234663852886e38)


def pack_keys(coords):
    """int64 keys of brick coordinates [n,3] (csrc/sparse_grid.h): ascending keys are the bricks in lexicographic (x, y, z) order."""
    c = np.asarray(coords, dtype=np.int64).reshape(-1, 3) + BRICK_LIMIT
    return (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]


def unpack_keys(keys):
    k = np.asarray(keys, dtype=np.int64).reshape(-1)
    return np.stack([(k >> 42) & 0x1fffff, (k >> 21) & 0x1fffff, k & 0x1fffff], axis=1).astype(np.int64) - BRICK_LIMIT


def _pixel_ranges(depth, K, pose, origin, voxel_size, trunc, max_depth):
    """(valid [P] bool, rejected [P] bool, lo [P,17,3] int64, hi [P,17,3] int64, k [P] int): the brick ranges of every sample of every
    pixel (row-major pixels); entries of pixels that are not valid, and of samples beyond k, are meaningless."""
    f32 = np.float32
    d = np.array(depth, dtype=f32)
    if d.ndim != 2:
        raise ValueError(f"mark_bricks: depth must be [h,w], got {d.shape}")
    h, w = d.shape
    K, P = np.asarray(K, dtype=f32).reshape(3, 3), np.asarray(pose, dtype=f32).reshape(4, 4)
    o = np.asarray(origin, dtype=f32).reshape(3)
    s, trunc, max_depth = f32(voxel_size), f32(trunc), f32(max_depth)
    if not s > 0 or not trunc > 0 or max_depth != max_depth:
        raise ValueError("mark_bricks: voxel_size and trunc must be positive and max_depth not NaN")
    with np.errstate(all="ignore"):
        d = d.reshape(-1).copy()
        d[d > max_depth] = f32(0)
        valid = (d > f32(0)) & (d <= _F32_MAX)
        d = np.where(valid, d, f32(1))
        v, u = np.divmod(np.arange(h * w), w)
        fx, cx, fy, cy = K[0, 0], K[0, 2], K[1, 1], K[1, 2]
        z0 = np.maximum(d - trunc, f32(0))
        z1 = d + trunc
        span = z1 - z0
        kf = np.minimum(np.maximum(np.ceil(span / (f32(2) * s)), f32(1)), f32(MAX_INTERVALS))
        delta = span / kf
        k = kf.astype(np.int64)
        a = (u.astype(f32) - cx) / fx
        b = (v.astype(f32) - cy) / fy
        ifx, ify = f32(1) / fx, f32(1) / fy
        r_pix = np.sqrt(ifx * ifx + ify * ify)
        r_ray = np.sqrt((f32(1) + a * a) + b * b)
        hd = f32(0.5) * delta
        t = P[:3, 3]
        W = (((np.abs(o[0]) + np.abs(o[1])) + np.abs(o[2])) + ((np.abs(t[0]) + np.abs(t[1])) + np.abs(t[2]))) + z1 * ((f32(1) + np.abs(a)) + np.abs(b))
        slack = SLACK_VOXELS * s + SLACK_RELATIVE * W
        brick = f32(8) * s
        n = MAX_INTERVALS + 1
        lo = np.zeros((h * w, n, 3), dtype=np.int64)
        hi = np.zeros((h * w, n, 3), dtype=np.int64)
        bad = np.zeros(h * w, dtype=bool)
        for i in range(n):
            z = z0 + f32(i) * delta
            m = ((HALF_PIXEL * (z + hd)) * r_pix + hd * r_ray) + slack
            x, y = a * z, b * z
            live = valid & (i <= k)
            for c in range(3):
                S = ((P[c, 0] * x + P[c, 1] * y) + P[c, 2] * z) + t[c]
                qlo = np.floor(((S - m) - o[c]) / brick)
                qhi = np.floor(((S + m) - o[c]) / brick)
                ok = (qlo >= f32(-BRICK_LIMIT)) & (qhi <= f32(BRICK_LIMIT)) & (qhi - qlo <= f32(MAX_SPAN - 1))    # False for NaN
                bad |= live & ~ok
                lo[:, i, c] = np.where(ok, qlo, f32(0)).astype(np.int64)
                hi[:, i, c] = np.where(ok, qhi, f32(0)).astype(np.int64)
    return valid & ~bad, valid & bad, lo, hi, k


def mark_bricks(depth, K, pose, origin, voxel_size, trunc, max_depth=np.inf, return_rejected=False):
    """Sorted unique brick coordinates [n,3] int32 (lexicographic in x, y, z) that the frame marks: the definition of marking (the module's
    docstring).  ``depth`` [h,w], ``K`` [3,3], camera-to-world ``pose`` [4,4], lattice ``origin`` [3].  ``return_rejected``: also the
    number of pixels that marked nothing because a sample left the coordinate range or spanned more than 4 bricks."""
    valid, rejected, lo, hi, k = _pixel_ranges(depth, K, pose, origin, voxel_size, trunc, max_depth)
    keys = []
    for i in range(MAX_INTERVALS + 1):
        live = valid & (i <= k)
        if not live.any():
            continue
        l, h = lo[live, i], hi[live, i]
        for dx in range(MAX_SPAN):
            for dy in range(MAX_SPAN):
                for dz in range(MAX_SPAN):
                    c = l + np.array([dx, dy, dz])
                    inside = (c <= h).all(axis=1)
                    if inside.any():
                        keys.append(np.unique(pack_keys(c[inside])))
    keys = np.unique(np.concatenate(keys)) if keys else np.zeros(0, dtype=np.int64)
    coords = unpack_keys(keys).astype(np.int32)
    return (coords, int(rejected.sum())) if return_rejected else coords


def brick_births(depths, K, poses, origin, voxel_size, trunc, max_depth=np.inf, first_frame=0):
    """(coords [n,3] int32 sorted lexicographically, birth [n] int32) for a sequence of frames numbered ``first_frame``, ``first_frame`` + 1,
    ...: a brick's birth is the number of the first frame that marks it.  ``K`` [3,3] for all frames or [N,3,3]."""
    K = np.asarray(K, dtype=np.float32)
    born = {}
    for f, (depth, pose) in enumerate(zip(depths, poses)):
        for key in pack_keys(mark_bricks(depth, K if K.ndim == 2 else K[f], pose, origin, voxel_size, trunc, max_depth)).tolist():
            born.setdefault(key, first_frame + f)
    keys = np.array(sorted(born), dtype=np.int64)
    return unpack_keys(keys).astype(np.int32), np.array([born[key] for key in keys.tolist()], dtype=np.int32)


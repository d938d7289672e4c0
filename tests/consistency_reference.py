"""Numpy restatement of the depth-map consistency filter (include/dvmvs_hip.h, "Depth-map consistency"), the scenes its tests share,
the ambiguity rule and the caps on the inputs.  Test infrastructure only.

``consistency_matrices`` restates step A (float64 from the float32 inputs, the header's operation order, each matrix rounded once to
float32).  ``depth_consistency`` restates step B for one dtype: with ``np.float32`` it follows the contract operation by operation (numpy
rounds every element-wise operation and never contracts), so the kernel is pinned against it bit for bit; with ``np.float64`` it evaluates
the same procedure from the same float32 inputs (the float32 matrices included) and can return the ambiguity flags.

Ambiguity rule: a pixel is ambiguous when, for any of its slots, |p.z| or |q.z| < 1e-4; us is within 1e-3 of 0 or W-1, or vs within 1e-3 of
0 or H-1; the validity of the four taps changes when the sample is shifted by +-1e-3 px along an axis; or the reprojection error is within
1e-3 px of the threshold while the relative difference is below its threshold + 1e-5, or the converse.
"""
import functools

import numpy as np

MAX_SOURCES = 16


def skipped(s, r, n):
    return s < 0 or s >= n or s == r


def _pair(Ka, Pa, Kb, Pb):
    """(A row-major, b) float64 [12] for "frame a's pixels to frame b's": the header's operation order, term by term."""
    Ka, Pa, Kb, Pb = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (Ka, Pa, Kb, Pb))
    Ra, ta, Rb, tb = Pa[:3, :3], Pa[:3, 3], Pb[:3, :3], Pb[:3, 3]
    fxa, fya, cxa, cya = Ka[0, 0], Ka[1, 1], Ka[0, 2], Ka[1, 2]
    fxb, fyb, cxb, cyb = Kb[0, 0], Kb[1, 1], Kb[0, 2], Kb[1, 2]
    R, t = np.empty((3, 3)), np.empty(3)
    for i in range(3):
        for j in range(3):
            R[i, j] = (Rb[0, i] * Ra[0, j] + Rb[1, i] * Ra[1, j]) + Rb[2, i] * Ra[2, j]
        ti = -((Rb[0, i] * tb[0] + Rb[1, i] * tb[1]) + Rb[2, i] * tb[2])
        t[i] = ((Rb[0, i] * ta[0] + Rb[1, i] * ta[1]) + Rb[2, i] * ta[2]) + ti
    ifx, ify, k02, k12 = 1.0 / fxa, 1.0 / fya, -(cxa / fxa), -(cya / fya)
    M = np.empty((3, 3))
    for j in range(3):
        M[0, j] = fxb * R[0, j] + cxb * R[2, j]
        M[1, j] = fyb * R[1, j] + cyb * R[2, j]
        M[2, j] = R[2, j]
    out = np.empty(12)
    for i in range(3):
        out[i * 3 + 0] = M[i, 0] * ifx
        out[i * 3 + 1] = M[i, 1] * ify
        out[i * 3 + 2] = (M[i, 0] * k02 + M[i, 1] * k12) + M[i, 2]
    out[9] = fxb * t[0] + cxb * t[2]
    out[10] = fyb * t[1] + cyb * t[2]
    out[11] = t[2]
    return out


def consistency_matrices(K, poses, sources):
    """Step A: float32 [N,S,2,12]; a skipped slot is zeros."""
    K, poses, sources = np.asarray(K, np.float32), np.asarray(poses, np.float32), np.asarray(sources, np.int32)
    n, S = sources.shape
    out = np.zeros((n, S, 2, 12), np.float32)
    with np.errstate(all="ignore"):
        for r in range(n):
            for j in range(S):
                s = int(sources[r, j])
                if skipped(s, r, n):
                    continue
                out[r, j, 0] = _pair(K[r], poses[r], K[s], poses[s]).astype(np.float32)
                out[r, j, 1] = _pair(K[s], poses[s], K[r], poses[r]).astype(np.float32)
    return out


def _valid(t):
    return np.isfinite(t) & (t > 0)


def depth_consistency(depths, K, poses, sources, pixel_threshold=1.0, relative_threshold=0.01, min_views=2, average=True,
                      dtype=np.float32, flags=False, matrices=None):
    """Step B in ``dtype``.  Returns a dict: ``depth`` [N,H,W], ``count`` uint8 [N,H,W], ``points`` [N,H,W,3], ``fused`` [N,H,W] (step 5's
    value whatever ``min_views``; 0 for an invalid d) and, with ``flags``, ``ambiguous`` bool [N,H,W]."""
    f = dtype
    depths, K, poses = np.asarray(depths, np.float32), np.asarray(K, np.float32), np.asarray(poses, np.float32)
    sources = np.asarray(sources, np.int32).reshape(depths.shape[0], -1)
    N, H, W = depths.shape
    S = sources.shape[1]
    if matrices is None:
        matrices = consistency_matrices(K, poses, sources)
    vv, uu = np.mgrid[0:H, 0:W]
    u, v = uu.astype(f), vv.astype(f)
    thr2 = f(pixel_threshold) * f(pixel_threshold)
    rel_thr = f(relative_threshold)
    count = np.zeros((N, H, W), np.int32)
    fused = np.zeros((N, H, W), f)
    amb = np.zeros((N, H, W), bool)
    with np.errstate(all="ignore"):
        for r in range(N):
            d = depths[r].astype(f)
            okr = _valid(d)
            acc = d.copy()
            for j in range(S):
                s = int(sources[r, j])
                if skipped(s, r, N) or H < 2 or W < 2:
                    continue
                m = matrices[r, j, 0].astype(f)
                m2 = matrices[r, j, 1].astype(f)
                px = d * ((m[0] * u + m[1] * v) + m[2]) + m[9]
                py = d * ((m[3] * u + m[4] * v) + m[5]) + m[10]
                pz = d * ((m[6] * u + m[7] * v) + m[8]) + m[11]
                us, vs = px / pz, py / pz
                inside = okr & (pz > 0) & (us >= 0) & (us <= f(W - 1)) & (vs >= 0) & (vs <= f(H - 1))
                usc, vsc = np.where(inside, us, f(0)), np.where(inside, vs, f(0))
                x0 = np.minimum(np.floor(usc), f(W - 2))
                y0 = np.minimum(np.floor(vsc), f(H - 2))
                wx, wy = usc - x0, vsc - y0
                xi, yi = x0.astype(np.int64), y0.astype(np.int64)
                src = depths[s].astype(f)
                t00, t01, t10, t11 = src[yi, xi], src[yi, xi + 1], src[yi + 1, xi], src[yi + 1, xi + 1]
                taps = _valid(t00) & _valid(t01) & _valid(t10) & _valid(t11)
                top = t00 + wx * (t01 - t00)
                bot = t10 + wx * (t11 - t10)
                ds = top + wy * (bot - top)
                qx = ds * ((m2[0] * usc + m2[1] * vsc) + m2[2]) + m2[9]
                qy = ds * ((m2[3] * usc + m2[4] * vsc) + m2[5]) + m2[10]
                qz = ds * ((m2[6] * usc + m2[7] * vsc) + m2[8]) + m2[11]
                du, dv = qx / qz - u, qy / qz - v
                e2 = du * du + dv * dv
                rel = np.abs(qz - d) / d
                ok = inside & taps & (qz > 0) & (e2 < thr2) & (rel < rel_thr)
                count[r] += ok
                acc = np.where(ok, acc + qz, acc)
                if flags:
                    a = okr & (np.abs(pz) < 1e-4)
                    for lim in (0, W - 1):
                        a |= okr & (pz > 0) & (np.abs(us - lim) < 1e-3)
                    for lim in (0, H - 1):
                        a |= okr & (pz > 0) & (np.abs(vs - lim) < 1e-3)
                    for sx, sy in ((1e-3, 0), (-1e-3, 0), (0, 1e-3), (0, -1e-3)):
                        xs, ys = np.clip(usc + sx, 0, W - 1), np.clip(vsc + sy, 0, H - 1)
                        xx = np.minimum(np.floor(xs).astype(np.int64), W - 2)
                        yy = np.minimum(np.floor(ys).astype(np.int64), H - 2)
                        shifted = _valid(src[yy, xx]) & _valid(src[yy, xx + 1]) & _valid(src[yy + 1, xx]) & _valid(src[yy + 1, xx + 1])
                        a |= inside & (shifted != taps)
                    e = np.sqrt(e2)
                    a |= inside & taps & (np.abs(qz) < 1e-4)
                    a |= inside & taps & (qz > 0) & (np.abs(e - pixel_threshold) < 1e-3) & (rel < relative_threshold + 1e-5)
                    a |= inside & taps & (qz > 0) & (np.abs(rel - relative_threshold) < 1e-5) & (e < pixel_threshold + 1e-3)
                    amb[r] |= a
            count[r] = np.where(okr, count[r], 0)
            fused[r] = np.where(okr, acc / (count[r] + 1).astype(f), f(0))
        dz = depths.astype(f)
        valid = _valid(dz)
        z = np.where(valid & (count >= min_views), fused if average else dz, f(0)).astype(f)
        # world position at z: the header's fp32 order
        points = np.zeros((N, H, W, 3), f)
        for r in range(N):
            Kr, P = K[r].astype(f), poses[r].astype(f)
            xn = (u - Kr[0, 2]) / Kr[0, 0]
            yn = (v - Kr[1, 2]) / Kr[1, 1]
            X, Y, Z = z[r] * xn, z[r] * yn, z[r]
            for i in range(3):
                c = ((P[i, 0] * X + P[i, 1] * Y) + P[i, 2] * Z) + P[i, 3]
                points[r, ..., i] = np.where(z[r] > 0, c, f(0))
    result = {"depth": z, "count": count.astype(np.uint8), "points": points, "fused": fused}
    if flags:
        result["ambiguous"] = amb
    return result


# ---- the shared scenes ---------------------------------------------------------------------------------------------------------------
def _rot_y(a):
    c, s = np.cos(a), np.sin(a)
    m = np.eye(4)
    m[:3, :3] = [[c, 0, -s], [0, 1, 0], [s, 0, c]]
    return m


def _rot_x(a):
    c, s = np.cos(a), np.sin(a)
    m = np.eye(4)
    m[:3, :3] = [[1, 0, 0], [0, c, -s], [0, s, c]]
    return m


def _tr(x, y, z):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    return m


def intrinsics(h, w, focal):
    return np.array([[focal, 0, (w - 1) / 2], [0, focal, (h - 1) / 2], [0, 0, 1]], dtype=np.float32)


PLANE_Z, SPHERE_CENTRE, SPHERE_RADIUS = 2.2, np.array([0.1, 0.0, 1.6]), 0.35


def render(K, P, h, w):
    """Exact depth, per pixel ray, of the plane z = 2.2 and the sphere in front of it, from the camera-to-world pose P."""
    K, P = K.astype(np.float64), P.astype(np.float64)
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    ray = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], -1)      # z = 1: the ray parameter is the depth
    o, D = P[:3, 3], ray @ P[:3, :3].T
    with np.errstate(all="ignore"):
        t_plane = (PLANE_Z - o[2]) / D[..., 2]
        t_plane[~(t_plane > 0)] = np.inf
        oc = o - SPHERE_CENTRE
        a, b, c = (D * D).sum(-1), 2 * (D @ oc), oc @ oc - SPHERE_RADIUS ** 2
        disc = b * b - 4 * a * c
        t_sphere = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf)
        t_sphere[~(t_sphere > 0)] = np.inf
    t = np.minimum(t_plane, t_sphere)
    t[~np.isfinite(t)] = 0
    return t.astype(np.float32)


def camera_poses():
    """Six cameras around the origin, 0.15 - 0.3 m apart, rotated by at most 0.13 rad."""
    return np.stack([_tr(0, 0, 0), _tr(0.15, 0.02, 0.0) @ _rot_y(0.06), _tr(-0.12, 0.05, 0.03) @ _rot_y(-0.05) @ _rot_x(0.03),
                     _tr(0.3, -0.04, 0.05) @ _rot_y(0.13), _tr(-0.28, 0.0, -0.05) @ _rot_y(-0.11),
                     _tr(0.05, 0.2, 0.1) @ _rot_x(0.1)]).astype(np.float32)


SIZES = {"24x32": (24, 32, 30.0), "23x37": (23, 37, 33.0), "64x80": (64, 80, 75.0)}
# four slots per frame; a -1 (frame 1), a frame's own index (frame 4) and an index >= N (frame 5) are skipped
SOURCES = np.array([[1, 2, 3, 4], [0, 2, 3, -1], [0, 1, 4, 5], [0, 1, 2, 4], [0, 4, 2, 3], [0, 1, 2, 6]], dtype=np.int32)
PATCH = (3, slice(5, 12), slice(8, 16))      # the 7x8 patch of view 3 that is scaled by 1.05
HOLED_VIEW, BROKEN_VIEW = 2, 4


@functools.lru_cache(maxsize=None)
def clean_scene(name):
    h, w, focal = SIZES[name]
    poses = camera_poses()
    K = np.stack([intrinsics(h, w, focal)] * len(poses))
    depths = np.stack([render(K[i], poses[i], h, w) for i in range(len(poses))])
    for a in (depths, K, poses):
        a.setflags(write=False)
    return depths, K, poses


@functools.lru_cache(maxsize=None)
def scene(name):
    """(depths [6,H,W], K [6,3,3], poses [6,4,4], sources [6,4]) with the defects: read-only, shared by the tests."""
    clean, K, poses = clean_scene(name)
    h, w = clean.shape[1:]
    depths = clean.copy()
    rng = np.random.default_rng(1)
    depths[HOLED_VIEW][rng.random((h, w)) < 0.1] = 0
    depths[PATCH] *= np.float32(1.05)
    depths[BROKEN_VIEW, 0, 0], depths[BROKEN_VIEW, 1, 1], depths[BROKEN_VIEW, 2, 2] = np.nan, np.inf, -1.0
    depths.setflags(write=False)
    SOURCES.setflags(write=False)
    return depths, K, poses, SOURCES


@functools.lru_cache(maxsize=None)
def scene_result(name, dtype_name):
    """The restatement's result on a shipped scene with the default thresholds (min_views 2, average): computed once and shared."""
    depths, K, poses, sources = scene(name)
    result = depth_consistency(depths, K, poses, sources, dtype=np.dtype(dtype_name).type, flags=dtype_name == "float64")
    for a in result.values():
        a.setflags(write=False)
    return result


CAP_AMBIGUOUS_SHARE, CAP_KEPT_SHARE = 0.01, 0.60


def check_caps(name):
    """The conditions on the INPUTS, from the float64 result alone; returns the figures."""
    depths = scene(name)[0]
    r64 = scene_result(name, "float64")
    valid = _valid(depths)
    ambiguous = r64["ambiguous"].reshape(len(depths), -1).mean(1)
    kept = float(((r64["count"] >= 2) & valid).sum() / valid.sum())
    patch_kept = int((r64["count"][PATCH] >= 2).sum())
    assert ambiguous.max() <= CAP_AMBIGUOUS_SHARE, f"{name}: {ambiguous.max():.4f} of a frame's pixels are ambiguous"
    assert kept >= CAP_KEPT_SHARE, f"{name}: only {kept:.3f} of the valid pixels have count >= 2"
    assert patch_kept == 0, f"{name}: {patch_kept} pixels of the scaled patch have count >= 2"
    return {"ambiguous": ambiguous, "kept": kept, "patch_kept": patch_kept}

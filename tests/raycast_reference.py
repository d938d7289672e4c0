"""Reference for the TSDF ray-caster (csrc/tsdf_raycast.hip): a vectorised numpy restatement of the definition in
include/dvmvs_hip.h, evaluated in float32 or float64, the rule for which pixels float32 may legitimately decide differently, and the
scenes the CPU and GPU tests share.  A plain helper module (no test module imports another).

``raycast(..., dtype=np.float32)`` follows the kernel operation by operation (same order, every operation rounded to ``dtype``).
``raycast(..., dtype=np.float64)`` evaluates the same procedure from the same float32 inputs and also returns the ambiguity flags.

A pixel is AMBIGUOUS (its hit / miss decision or its bracket may differ between correct float32 evaluations) when
  * among its samples up to the hit (all of them on a miss) one is valid with |f| < 1e-5, or
  * one of those samples changes validity when shifted by +-1e-4 voxel along an axis, or
  * (z1 - z0) / dz is within 1e-3 of an integer (the number of samples is undecided), or |z1 - z0| < 1e-6 (the ray grazes the box).
Normals are further excluded where one of the six gradient samples changes validity under the same shifts or the gradient norm is
below 1e-3; colours where the hit point lies within 1e-4 voxel of a rounding boundary.

The caps are conditions on the INPUTS, computed from the float64 result alone (``check_caps``): at most 3 % ambiguous pixels per view,
at most a further 3 % of the hit pixels excluded for normals and the same for colours, at least 20 % hits in a view meant to see the
surface.  An input that breaks a cap is replaced, never the cap.
"""
import functools
from types import SimpleNamespace

import numpy as np

AMBIGUOUS_CAP, EXCLUDED_CAP, HIT_FLOOR = 0.03, 0.03, 0.20
F_EPS, SHIFT, COUNT_EPS, GRAZE_EPS, NORM_EPS, ROUND_EPS = 1e-5, 1e-4, 1e-3, 1e-6, 1e-3, 1e-4
TRUNC_VOXELS = 5.0
VOXEL = float(np.float32(0.05))      # the float32 the kernel receives


def _lerp(a, b, w):
    return a * (w.dtype.type(1.0) - w) + b * w


def _clamp(g, dims):
    return np.minimum(np.maximum(g, g.dtype.type(0.0)), (dims - 1).astype(g.dtype))


def _cell(g, dims):
    return np.maximum(np.minimum(np.floor(g).astype(np.int64), dims - 2), 0)


def _corners(vol, c):
    return [vol[c[:, 0] + ((i >> 2) & 1), c[:, 1] + ((i >> 1) & 1), c[:, 2] + (i & 1)] for i in range(8)]


def _valid(weight, g, dims):
    w = _corners(weight, _cell(g, dims))
    return np.logical_and.reduce([x > 0 for x in w])


def _sample(tsdf, weight, g, dims):
    """(trilinear tsdf, validity) at the clamped points g [P,3]: z, then y, then x, as the kernel."""
    c = _cell(g, dims)
    w = g - c.astype(g.dtype)
    t = _corners(tsdf, c)
    valid = np.logical_and.reduce([x > 0 for x in _corners(weight, c)])
    c00, c01, c10, c11 = (_lerp(t[0], t[1], w[:, 2]), _lerp(t[2], t[3], w[:, 2]), _lerp(t[4], t[5], w[:, 2]), _lerp(t[6], t[7], w[:, 2]))
    return _lerp(_lerp(c00, c01, w[:, 1]), _lerp(c10, c11, w[:, 1]), w[:, 0]), valid


def _validity_moves(weight, g, valid, dims):
    """True where the validity of the sample at g changes under a shift of +-SHIFT voxel along an axis."""
    moved = np.zeros(len(g), dtype=bool)
    for a in range(3):
        for s in (-SHIFT, SHIFT):
            gs = g.copy()
            gs[:, a] += s
            moved |= _valid(weight, _clamp(gs, dims), dims) != valid
    return moved


def decode_color(col):
    """Folded b * 65536 + g * 256 + r (float32) -> uint8 [...,3] RGB, the float32 arithmetic of marching_cubes.hip."""
    col = np.asarray(col, dtype=np.float32)
    b = np.floor(col / np.float32(65536.0))
    g = np.floor((col - b * np.float32(65536.0)) / np.float32(256.0))
    r = col - b * np.float32(65536.0) - g * np.float32(256.0)
    return np.stack([np.floor(r), np.floor(g), np.floor(b)], axis=-1).astype(np.uint8)


def brick_mask(tsdf, weight):
    """The brick mask's definition, corner by corner: one flag per 8x8x8 block of cells, set when a corner of one of its cells has
    weight > 0 and tsdf <= 0 (a block's cells 8b .. 8b+7 have the corners 8b .. 8b+8)."""
    crossing = (np.asarray(weight) > 0) & (np.asarray(tsdf) <= 0)
    shape = tuple(-(-(d - 1) // 8) for d in crossing.shape)
    mask = np.zeros(shape, dtype=np.uint8)
    for b in np.ndindex(*shape):
        mask[b] = crossing[8 * b[0]:8 * b[0] + 9, 8 * b[1]:8 * b[1] + 9, 8 * b[2]:8 * b[2] + 9].any()
    return mask


def n_cap(dims, step):
    d = np.asarray(dims, dtype=np.float64) - 1.0
    return int(np.floor(np.sqrt((d * d).sum()) / float(np.float32(step))) + 2.0)


def raycast(tsdf, weight, color, origin, voxel_size, cam_intr, cam_pose, height, width, near=0.0, far=np.inf, step=1.0, dtype=np.float64):
    """The ray-caster's definition in ``dtype``.  Volumes [X,Y,Z]; ``tsdf`` is converted to ``dtype`` (a float64 volume stays exact in
    float64), every other input is rounded to float32 first -- what the kernel receives -- and then converted.  ``cam_intr`` [N,3,3] or
    [3,3], ``cam_pose`` [N,4,4] or [4,4].  Returns a namespace of [N,H,W(,3)] arrays: depth, hit, normal, rgb, n_samples and, in
    float64, ambiguous, normal_excluded, colour_excluded."""
    T = np.dtype(dtype).type
    flags = T is np.float64
    tsdf = np.asarray(tsdf).astype(T)
    weight = np.asarray(weight, dtype=np.float32)
    dims = np.array(tsdf.shape, dtype=np.int64)
    hi = (dims - 1).astype(T)
    origin = np.asarray(origin, dtype=np.float32).astype(T)
    vs, near_t, far_t, step_t = (T(np.float32(x)) for x in (voxel_size, near, far, step))
    poses = np.asarray(cam_pose, dtype=np.float32).reshape(-1, 4, 4).astype(T)
    Ks = np.asarray(cam_intr, dtype=np.float32).reshape(-1, 3, 3).astype(T)
    if len(Ks) == 1:
        Ks = np.repeat(Ks, len(poses), 0)
    cap = n_cap(dims, step)
    N, P = len(poses), height * width
    out = SimpleNamespace(depth=np.zeros((N, P), T), hit=np.zeros((N, P), bool), normal=np.zeros((N, P, 3), T),
                          rgb=np.zeros((N, P, 3), np.uint8), n_samples=np.zeros((N, P), np.int64), ambiguous=np.zeros((N, P), bool),
                          normal_excluded=np.zeros((N, P), bool), colour_excluded=np.zeros((N, P), bool))
    vv, uu = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    u, v = uu.reshape(-1).astype(T), vv.reshape(-1).astype(T)
    with np.errstate(all="ignore"):
        for i in range(N):
            K, R, t = Ks[i], poses[i, :3, :3], poses[i, :3, 3]
            dcx, dcy = (u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1]
            og = np.broadcast_to(((t - origin) / vs)[None, :], (P, 3)).copy()
            dg = np.stack([((R[a, 0] * dcx + R[a, 1] * dcy) + R[a, 2]) / vs for a in range(3)], axis=1)
            ok = np.isfinite(og).all(1) & np.isfinite(dg).all(1)
            tmin, tmax = np.full(P, -np.inf, T), np.full(P, np.inf, T)
            for a in range(3):
                zero = dg[:, a] == 0
                ok &= ~zero | ((og[:, a] >= 0) & (og[:, a] <= hi[a]))
                ta, tb = (T(0.0) - og[:, a]) / dg[:, a], (hi[a] - og[:, a]) / dg[:, a]
                tmin = np.where(zero, tmin, np.maximum(tmin, np.minimum(ta, tb)))
                tmax = np.where(zero, tmax, np.minimum(tmax, np.maximum(ta, tb)))
            z0, z1 = np.maximum(tmin, near_t), np.minimum(tmax, far_t)
            length = np.sqrt((dg[:, 0] * dg[:, 0] + dg[:, 1] * dg[:, 1]) + dg[:, 2] * dg[:, 2])
            dz = step_t / length
            ok &= np.isfinite(z0) & np.isfinite(z1) & (z0 <= z1) & np.isfinite(dz) & (dz > 0)
            q = np.where(ok, (z1 - z0) / dz, T(-1.0))
            n = np.where(ok, np.minimum(np.floor(q), T(cap)), T(-1.0)).astype(np.int64)
            out.n_samples[i] = n + 1
            amb = np.zeros(P, bool)
            if flags:
                amb |= ok & (np.abs(q - np.rint(q)) < COUNT_EPS)
                amb |= np.isfinite(z0) & np.isfinite(z1) & (np.abs(z1 - z0) < GRAZE_EPS)
            hit = np.zeros(P, bool)
            depth = np.zeros(P, T)
            prev_f, prev_valid = np.zeros(P, T), np.zeros(P, bool)
            for k in range(int(n.max()) + 1 if ok.any() else 0):
                act = ok & ~hit & (k <= n)
                g = _clamp(og + (z0 + T(k) * dz)[:, None] * dg, dims)
                f, valid = _sample(tsdf, weight, g, dims)
                if flags:
                    amb |= act & valid & (np.abs(f) < F_EPS)
                    amb |= act & _validity_moves(weight, g, valid, dims)
                if k >= 1:
                    new = act & valid & (f <= 0) & prev_valid & (prev_f > 0)
                    d = (z0 + T(k - 1) * dz) + dz * (prev_f / (prev_f - f))
                    depth = np.where(new, d, depth)
                    hit |= new
                prev_f, prev_valid = f, valid
            hit &= depth != 0
            out.depth[i], out.hit[i], out.ambiguous[i] = depth, hit, amb
            # normal and colour at the hit point
            gs = _clamp(og + depth[:, None] * dg, dims)
            nrm = np.zeros((P, 3), T)
            all_valid = np.ones(P, bool)
            moved = np.zeros(P, bool)
            for a in range(3):
                gp, gm = gs.copy(), gs.copy()
                gp[:, a] = np.minimum(gs[:, a] + T(1.0), hi[a])
                gm[:, a] = np.maximum(gs[:, a] - T(1.0), T(0.0))
                fp, vp = _sample(tsdf, weight, gp, dims)
                fm, vm = _sample(tsdf, weight, gm, dims)
                nrm[:, a] = fp - fm
                all_valid &= vp & vm
                if flags:
                    moved |= _validity_moves(weight, gp, vp, dims) | _validity_moves(weight, gm, vm, dims)
            nlen = np.sqrt((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2])
            keep = hit & all_valid & (nlen > 0) & np.isfinite(nlen)
            out.normal[i] = np.where(keep[:, None], nrm / nlen[:, None], T(0.0))
            qi = np.clip(np.rint(gs).astype(np.int64), 0, dims - 1)
            if color is not None:
                out.rgb[i] = np.where(hit[:, None], decode_color(np.asarray(color, dtype=np.float32)[qi[:, 0], qi[:, 1], qi[:, 2]]), 0)
            if flags:
                out.normal_excluded[i] = hit & (moved | (nlen < NORM_EPS))
                out.colour_excluded[i] = hit & (np.abs((gs - np.floor(gs)) - 0.5) < ROUND_EPS).any(1)
    for name, value in vars(out).items():
        setattr(out, name, value.reshape((N, height, width) + value.shape[2:]))
    return out


def check_caps(ref, sees_surface=True):
    """The conditions on the inputs, from the float64 result alone.  Returns the per-view shares for printing."""
    shares = []
    for i in range(len(ref.depth)):
        hits = ref.hit[i] & ~ref.ambiguous[i]
        amb, hit = ref.ambiguous[i].mean(), ref.hit[i].mean()
        n_ex = (hits & ref.normal_excluded[i]).sum() / max(hits.sum(), 1)
        c_ex = (hits & ref.colour_excluded[i]).sum() / max(hits.sum(), 1)
        shares.append((amb, hit, n_ex, c_ex))
        assert amb <= AMBIGUOUS_CAP, f"view {i}: {100 * amb:.2f} % ambiguous pixels: replace the input"
        assert n_ex <= EXCLUDED_CAP and c_ex <= EXCLUDED_CAP, f"view {i}: {100 * n_ex:.2f} % / {100 * c_ex:.2f} % excluded: replace the input"
        if sees_surface:
            assert hit >= HIT_FLOOR, f"view {i}: only {100 * hit:.1f} % hits: replace the input"
    return shares


# ---- scenes -----------------------------------------------------------------------------------------------------------
DIMS_SMALL, DIMS_ODD = (24, 20, 16), (33, 29, 21)       # the second: odd, no multiple of the 8-cell brick
IMAGE_A, IMAGE_B = (24, 32), (17, 23)                   # both leave partial 8x8 tiles
PLANE_NORMAL = np.array([0.2, -0.3, -1.0]) / np.linalg.norm([0.2, -0.3, -1.0])


def _origin(dims):
    """Volume centred on the optical axis of the frontal camera, its near face at z = 0.8 m."""
    ext = (np.array(dims) - 1) * VOXEL
    return np.array([-ext[0] / 2, -ext[1] / 2, 0.8]).astype(np.float32)


def _world(dims):
    o = _origin(dims).astype(np.float64)
    ix, iy, iz = np.meshgrid(*[np.arange(d, dtype=np.float64) for d in dims], indexing="ij")
    return np.stack([o[0] + ix * VOXEL, o[1] + iy * VOXEL, o[2] + iz * VOXEL], axis=-1), (ix, iy, iz)


def _finish(dims, sd, hole=True):
    """float64 tsdf = min(1, sd / trunc), weight 1 where sd >= -trunc; a 4x5xZ column of unobserved voxels; a smooth colour pattern."""
    trunc = TRUNC_VOXELS * VOXEL
    tsdf = np.minimum(1.0, sd / trunc)
    weight = (sd >= -trunc).astype(np.float32)
    hole_at = None
    if hole:
        x0, y0 = dims[0] // 2 + 2, dims[1] // 2 - 6
        hole_at = (slice(x0, x0 + 4), slice(y0, y0 + 5), slice(None))
        tsdf[hole_at], weight[hole_at] = 1.0, 0.0
    _, (ix, iy, iz) = _world(dims)
    color = ((30 + 10 * iz) * 65536 + (20 + 8 * iy) * 256 + (10 + 7 * ix)).astype(np.float32)
    return SimpleNamespace(dims=tuple(dims), origin=_origin(dims), voxel_size=VOXEL, tsdf64=tsdf, tsdf=tsdf.astype(np.float32), weight=weight,
                           color=color, hole=hole_at)


def plane_volume(dims, hole=True):
    pts, _ = _world(dims)
    centre = _origin(dims).astype(np.float64) + (np.array(dims) - 1) * VOXEL / 2
    vol = _finish(dims, (pts - centre) @ PLANE_NORMAL, hole)       # positive on the cameras' side
    vol.plane_point, vol.plane_normal = centre, PLANE_NORMAL
    return vol


def sphere_volume(dims, hole=True):
    pts, _ = _world(dims)
    centre = _origin(dims).astype(np.float64) + (np.array(dims) - 1) * VOXEL / 2
    radius = (dims[2] - 1) * VOXEL / 3          # a third of the depth extent: at least 20 % of the pixels of every view below see it
    vol = _finish(dims, np.linalg.norm(pts - centre, axis=-1) - radius, hole)
    vol.centre, vol.radius = centre, radius
    return vol


def empty_volume(dims):
    """Nothing observed: tsdf 1, weight 0 everywhere."""
    vol = _finish(dims, np.full(dims, 10.0), hole=False)
    vol.weight = np.zeros(dims, np.float32)
    return vol


def intrinsics(image, integer_principal_point=False):
    h, w = image
    f = 26.3 * w / 32.0
    cx, cy = (w // 2, h // 2) if integer_principal_point else (w / 2 - 0.63, h / 2 - 0.39)
    return np.array([[f, 0, cx], [0, f * 0.955, cy], [0, 0, 1.0]], dtype=np.float32)


def _yaw(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def view(kind):
    """Camera-to-world poses (float32): the camera looks along +z; the volume's near face is at z = 0.8 m."""
    pose = np.eye(4)
    if kind == "frontal":            # 0.4 m in front of the volume
        pose[:3, 3] = [0.013, -0.021, 0.4]
    elif kind == "yaw+":
        pose[:3, :3], pose[:3, 3] = _yaw(0.2), [-0.18, 0.031, 0.4]
    elif kind == "yaw-inside":       # yawed the other way and shifted INTO the volume (5 cm behind its near face)
        pose[:3, :3], pose[:3, 3] = _yaw(-0.35), [0.22, -0.043, 0.85]
    elif kind == "parallel":         # identity rotation: with an integer principal point the centre row and column of rays have a
        pose[:3, 3] = [0.013, -0.021, 0.4]     # direction component that is exactly 0 (off-centre, or they would run along voxel-rounding boundaries)
    elif kind == "away":             # looks along -z, away from the volume
        pose[:3, :3], pose[:3, 3] = _yaw(np.pi), [0.0, 0.0, 0.4]
    else:
        raise KeyError(kind)
    return pose.astype(np.float32)


THREE_VIEWS = ("frontal", "yaw+", "yaw-inside")

# name -> (volume builder, dims, image, views, keyword arguments of the march)
CASES = {
    "plane_small_n3": (plane_volume, DIMS_SMALL, IMAGE_A, THREE_VIEWS, {}),
    "plane_odd_n1": (plane_volume, DIMS_ODD, IMAGE_B, ("frontal",), {}),
    "plane_odd_n3_half_step": (plane_volume, DIMS_ODD, IMAGE_A, THREE_VIEWS, {"step": 0.5}),
    "plane_small_n1_double_step": (plane_volume, DIMS_SMALL, IMAGE_B, ("yaw+",), {"step": 2.0}),
    "plane_small_near_far": (plane_volume, DIMS_SMALL, IMAGE_A, ("frontal",), {"near": 0.74, "far": 0.83}),
    "plane_small_parallel": (plane_volume, DIMS_SMALL, IMAGE_A, ("parallel",), {}),
    "sphere_small_n1": (sphere_volume, DIMS_SMALL, IMAGE_B, ("frontal",), {}),
    "sphere_small_n3_double_step": (sphere_volume, DIMS_SMALL, IMAGE_A, THREE_VIEWS, {"step": 2.0}),
    "sphere_odd_n3": (sphere_volume, DIMS_ODD, IMAGE_A, THREE_VIEWS, {}),
    "sphere_odd_n1_half_step": (sphere_volume, DIMS_ODD, IMAGE_B, ("yaw+",), {"step": 0.5}),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(volume, K [3,3], poses [N,4,4], (H, W), kwargs, float32 result, float64 result) of a named case; computed once per process."""
    builder, dims, image, views, kwargs = CASES[name]
    vol = builder(dims)
    K = intrinsics(image, integer_principal_point="parallel" in views)
    poses = np.stack([view(v) for v in views])
    args = (vol.tsdf, vol.weight, vol.color, vol.origin, vol.voxel_size, K, poses, image[0], image[1])
    return SimpleNamespace(name=name, vol=vol, K=K, poses=poses, image=image, kwargs=dict(kwargs),
                           ref32=raycast(*args, dtype=np.float32, **kwargs), ref64=raycast(*args, dtype=np.float64, **kwargs))


def plane_depth(vol, K, pose, height, width):
    """Closed form: camera depth at which each pixel's ray meets the plane of ``plane_volume`` (float64, from the float32 inputs)."""
    K, pose = np.asarray(K, np.float32).astype(np.float64), np.asarray(pose, np.float32).astype(np.float64)
    v, u = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    d = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], -1) @ pose[:3, :3].T
    return ((vol.plane_point - pose[:3, 3]) @ vol.plane_normal) / (d @ vol.plane_normal)


def voxel_points(vol, K, pose, depth):
    """Voxel coordinates [H,W,3] of the points at camera depth ``depth`` [H,W] along the pixels' rays (float64)."""
    K, pose = np.asarray(K, np.float32).astype(np.float64), np.asarray(pose, np.float32).astype(np.float64)
    h, w = depth.shape
    v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    d = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], -1) @ pose[:3, :3].T
    return (pose[:3, 3] + depth[..., None] * d - vol.origin.astype(np.float64)) / vol.voxel_size


@functools.lru_cache(maxsize=None)
def oracle_volume(n_frames=2):
    """Scene (c): the frames of ``synthetic.tsdf_inputs()`` integrated on the CPU by oracle/tsdf_oracle.py (weights 1, 2)."""
    import synthetic as syn
    import tsdf_oracle as tso
    frames, bounds, voxel = syn.tsdf_inputs()
    dims = tuple(int(d) for d in np.ceil((bounds[:, 1] - bounds[:, 0]) / voxel))
    tsdf, weight, color = np.ones(dims, np.float32), np.zeros(dims, np.float32), np.zeros(dims, np.float32)
    for n, (rgb, depth, K, pose) in enumerate(frames[:n_frames]):
        tso.integrate(tsdf, weight, color, bounds[:, 0], voxel, K, pose, tso.fold_color(rgb), depth, 5 * voxel, obs_weight=1.0 + n)
    return SimpleNamespace(dims=dims, origin=bounds[:, 0].astype(np.float32), voxel_size=float(voxel), tsdf=tsdf, weight=weight, color=color,
                           frames=frames, bounds=bounds)


@functools.lru_cache(maxsize=None)
def oracle_case(n_frames=2):
    """Scene (c) seen from its own frames' poses at the frames' size."""
    vol = oracle_volume(n_frames)
    K = np.stack([f[2] for f in vol.frames]).astype(np.float32)
    poses = np.stack([f[3] for f in vol.frames]).astype(np.float32)
    image = vol.frames[0][1].shape
    args = (vol.tsdf, vol.weight, vol.color, vol.origin, vol.voxel_size, K, poses, image[0], image[1])
    return SimpleNamespace(name=f"oracle_{n_frames}", vol=vol, K=K, poses=poses, image=image, kwargs={},
                           ref32=raycast(*args, dtype=np.float32), ref64=raycast(*args, dtype=np.float64))

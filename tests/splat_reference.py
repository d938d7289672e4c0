"""Float64 references for the two forward kernels that move geometry, and the inputs their tests share (a plain helper module
like accuracy.py: no fixtures, no test module imports another).

Depth re-projection.  ``splat_reference`` restates oracle/dvmvs_oracle.py:reproject_depth in float64 from a given
transformation and says, per source point, whether float32 arithmetic may legitimately put it somewhere else:

* a projected coordinate within ``DELTA`` px of a rounding boundary n + 0.5 (the image borders -0.5, hw - 0.5, hh - 0.5 are such
  boundaries), or
* ``|Z| < DELTA`` (the sign of z, and the ``|z| > 1e-8`` switch of the perspective divide), or
* a non-finite intermediate (an inf / nan depth: its coordinates are nan in any precision and it lands nowhere).

Every other point has one certain target cell.  Per target cell the reference keeps ``lo``, the largest relu(z) among the certain
points, and ``hi``, the largest among those plus every ambiguous point that could land there.  ``check_splat`` is the one
comparison rule: a cell without ambiguous candidates must hold ``lo`` (0 exactly where nothing lands); a cell with some must hold
one candidate's z inside [lo, hi].  Nothing is skipped and nothing is counted away.

``DELTA`` = 1e-3 px: the float32 round-off of a projected coordinate below 160 px is about 1e-4 px at worst.  The two caps are
conditions on the INPUTS (computed from the float64 reference alone, never from a kernel's output): at most 1 % ambiguous source
points and at most 5 % of the hit cells under the bracket rule.  An input that exceeds a cap is replaced, the cap is not.

TSDF integration.  ``tsdf_integrate`` is oracle/tsdf_oracle.py:integrate with a ``dtype`` argument; in float64 it tells, for a voxel
on which the kernel and the float32 oracle disagree, whether the voxel sits on a roundf tie or on the truncation edge (a badly chosen
input) or not (a kernel bug): ``tsdf_explain``.
"""
import math

import numpy as np
import torch

import dvmvs_oracle as orc
import synthetic as syn
from accuracy import as_accurate_as_reference

DELTA = 1e-3
MAX_AMBIGUOUS_POINTS = 0.01
MAX_BRACKETED_CELLS = 0.05
MIN_LANDING = 0.20
EPS = 1e-8            # kornia.convert_points_from_homogeneous
# Absolute float32 round-off of X, Y, Z (4-term dot products of terms below ~10 m: each of the ~7 roundings is at most 6e-7).  Only
# used to say where a point with |Z| < DELTA could land: its projection X / Z moves by this much divided by |Z|.
Z_ROUNDOFF = 1e-5


class SplatReference:
    """Per source point: ``u``, ``v`` (projected coordinates), ``cell_j``, ``cell_i`` (target column / row after half-to-even
    rounding, nan where non-finite), ``z`` (relu(z)), ``ambiguous``, ``lands`` (certainly or not: finite, inside, z > 0).  Per target cell [B,hh,hw]: ``lo``, ``hi``,
    ``bracketed``; ``exact`` is the plain float64 splat that ignores ambiguity.  ``candidates`` = (flat cell index over [B,hh,hw], z)
    of every point that may land on a cell."""


def splat_reference(T, depth, full_K, half_K, delta=DELTA):
    T, depth, full_K, half_K = (np.asarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype=np.float64)
                                for t in (T, depth, full_K, half_K))
    B, _, H, W = depth.shape
    hh, hw = H // 2, W // 2
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ref = SplatReference()
    ref.shape = (B, hh, hw)
    n_cells = hh * hw
    lo, hi, exact = (np.zeros(B * n_cells) for _ in range(3))
    bracketed = np.zeros(B * n_cells, dtype=bool)
    per_point = {k: np.zeros((B, H, W)) for k in ("cell_j", "cell_i", "z", "u", "v")}
    ambiguous, lands = np.zeros((B, H, W), dtype=bool), np.zeros((B, H, W), dtype=bool)
    cand_cell, cand_z = [], []
    with np.errstate(all="ignore"):
        for b in range(B):
            Kf, Kh, M = full_K[b], half_K[b], T[b]
            d = depth[b, 0]
            px, py = (xs - Kf[0, 2]) / Kf[0, 0] * d, (ys - Kf[1, 2]) / Kf[1, 1] * d
            q = [M[r, 0] * px + M[r, 1] * py + M[r, 2] * d + M[r, 3] for r in range(4)]
            sw = np.where(np.abs(q[3]) > EPS, 1.0 / q[3], 1.0)
            X, Y, Z = sw * q[0], sw * q[1], sw * q[2]
            z = np.where(Z > 0, Z, 0.0)                                    # relu; nan -> 0 (it lands nowhere)
            sz = np.where(np.abs(Z) > EPS, 1.0 / Z, 1.0)                   # the projection uses the un-clamped z
            u, v = X * sz * Kh[0, 0] + Kh[0, 2], Y * sz * Kh[1, 1] + Kh[1, 2]
            finite = np.isfinite(u) & np.isfinite(v) & np.isfinite(Z) & np.isfinite(q[3])
            near = lambda c: np.abs(c - np.floor(c) - 0.5) < delta
            tiny_z = finite & ((np.abs(Z) < delta) | (np.abs(q[3]) < delta))
            amb = ~finite | near(u) | near(v) | tiny_z
            j, i = np.rint(u), np.rint(v)                                  # half to even, like torch.round and rintf
            inside = finite & (j >= 0) & (j < hw) & (i >= 0) & (i < hh)
            per_point["cell_j"][b], per_point["cell_i"][b], per_point["z"][b] = np.where(finite, j, np.nan), np.where(finite, i, np.nan), z
            per_point["u"][b], per_point["v"][b] = u, v
            ambiguous[b], lands[b] = amb, inside & (z > 0)
            base = b * n_cells
            lin = (base + np.where(inside, i, 0) * hw + np.where(inside, j, 0)).astype(np.int64)
            np.maximum.at(exact, lin[inside], z[inside])
            sure = inside & ~amb & (z > 0)
            np.maximum.at(lo, lin[sure], z[sure])
            cand_cell.append(lin[sure])
            cand_z.append(z[sure])
            # ambiguous points: the cell(s) on either side of the boundary; with a tiny |Z| every cell the round-off of X / Z reaches
            for (yy, xx) in zip(*np.nonzero(amb & finite & ((z > 0) | tiny_z))):
                uu, vv, zz = u[yy, xx], v[yy, xx], abs(Z[yy, xx])
                ru = rv = delta
                if tiny_z[yy, xx]:
                    spread = Z_ROUNDOFF / zz if zz > Z_ROUNDOFF else math.inf
                    ru, rv = delta + (abs(uu - Kh[0, 2]) + abs(Kh[0, 0])) * spread, delta + (abs(vv - Kh[1, 2]) + abs(Kh[1, 1])) * spread
                j0, j1 = (max(0, int(np.rint(max(uu - ru, -1.0)))), min(hw - 1, int(np.rint(min(uu + ru, float(hw)))))) if math.isfinite(ru) else (0, hw - 1)
                i0, i1 = (max(0, int(np.rint(max(vv - rv, -1.0)))), min(hh - 1, int(np.rint(min(vv + rv, float(hh)))))) if math.isfinite(rv) else (0, hh - 1)
                if j0 > j1 or i0 > i1:
                    continue
                cells = (base + np.arange(i0, i1 + 1)[:, None] * hw + np.arange(j0, j1 + 1)[None, :]).reshape(-1)
                bracketed[cells] = True
                cand_cell.append(cells)
                cand_z.append(np.full(cells.shape, z[yy, xx]))
    hi[:] = lo
    ref.candidates = (np.concatenate(cand_cell), np.concatenate(cand_z))
    np.maximum.at(hi, ref.candidates[0], ref.candidates[1])
    ref.lo, ref.hi, ref.exact, ref.bracketed = (a.reshape(B, hh, hw) for a in (lo, hi, exact, bracketed))
    ref.cell_j, ref.cell_i, ref.z = per_point["cell_j"], per_point["cell_i"], per_point["z"]
    ref.u, ref.v = per_point["u"], per_point["v"]
    ref.ambiguous, ref.lands = ambiguous, lands
    hit = (ref.lo > 0) | ref.bracketed
    ref.ambiguous_share = float(ambiguous.mean())
    ref.bracketed_share = float(ref.bracketed.sum()) / max(1, int(hit.sum()))
    ref.landing_share = float(lands.mean())
    return ref


def check_splat(got, oracle32, ref, slack=3.0, floor=2e-6):
    """The comparison rule.  ``got`` / ``oracle32`` [B,1,hh,hw] float32 (the kernel's output, the float32 oracle's).  Returns
    (share of ambiguous source points, share of hit cells that took the bracket rule)."""
    got64 = got.detach().cpu().double().numpy().reshape(ref.shape)
    o64 = oracle32.detach().cpu().double().numpy().reshape(ref.shape)
    assert np.isfinite(got64).all(), "non-finite value in the splat"
    clean = ~ref.bracketed
    empty = clean & (ref.lo == 0)
    assert (got64[empty] == 0).all(), f"{int((got64[empty] != 0).sum())} cells that no point reaches are not 0"
    tol = floor
    if clean.any():
        as_accurate_as_reference(torch.from_numpy(got64[clean]), torch.from_numpy(o64[clean]), torch.from_numpy(ref.lo[clean]), slack, floor)
        tol = slack * float(np.abs(o64[clean] - ref.lo[clean]).max()) + floor
    br = ref.bracketed
    g, lo, hi = got64[br], ref.lo[br], ref.hi[br]
    assert (g >= lo - tol).all() and (g <= hi + tol).all(), \
        f"{int(((g < lo - tol) | (g > hi + tol)).sum())} bracketed cells outside [lo, hi] (tolerance {tol:.2e})"
    assert (lo[g == 0] == 0).all(), "a bracketed cell is empty although a certain point lands on it"
    # ... and the value is one candidate's z (0 = no candidate landed, only where lo == 0: checked above)
    flat = got64.reshape(-1)
    cells, zs = ref.candidates
    best = np.full(flat.shape, np.inf)
    np.minimum.at(best, cells, np.abs(flat[cells] - zs))
    best[flat == 0] = 0.0
    worst = best.reshape(ref.shape)[br]
    assert (worst <= tol).all(), f"{int((worst > tol).sum())} bracketed cells hold a value that is no candidate's z (off by up to {worst.max():.3e})"
    return ref.ambiguous_share, ref.bracketed_share


def assert_caps(ref, name, min_landing=MIN_LANDING):
    print(f"{name}: {100 * ref.ambiguous_share:.3f} % ambiguous source points, {100 * ref.bracketed_share:.3f} % of the hit cells bracketed, "
          f"{100 * ref.landing_share:.1f} % of the points land inside")
    assert ref.ambiguous_share <= MAX_AMBIGUOUS_POINTS, (name, ref.ambiguous_share)
    assert ref.bracketed_share <= MAX_BRACKETED_CELLS, (name, ref.bracketed_share)
    assert ref.landing_share >= min_landing, (name, ref.landing_share)


def oracle_splat(T, depth, full_K, half_K):
    """The float32 oracle from a given transformation: inverse(identity) @ T is T, bit for bit."""
    B, _, H, W = depth.shape
    return orc.reproject_depth(torch.eye(4).repeat(B, 1, 1), T, depth, full_K, half_K, W, H)


def decimated(full, f):
    """What F.interpolate(scale_factor=1/f, mode="nearest") keeps of the half-resolution map: rows / columns 0, f, 2f, ... that fit."""
    hh, hw = full.shape[-2:]
    return full[..., ::f, ::f][..., :hh // f, :hw // f].contiguous()


# ---- the case table (seeded, deterministic): shared by test_splat_reference.py (CPU) and test_geometry_kernels_gpu.py ---------------
FACTORS = (1, 2, 3, 5, 16)

# name: (height, width, batch, motion, depth kind, seed)
SPLAT_CASES = {
    "scene_256x320_smooth": (256, 320, 1, "scene", "smooth", 11),
    "scene_64x80_holes_b3": (64, 80, 3, "scene", "holes", 101),
    "scene_37x53_two_layer_b3": (37, 53, 3, "scene", "two_layer", 13),
    "scene_130x98_holes": (130, 98, 1, "scene", "holes", 105),
    "forward_256x320_two_layer": (256, 320, 1, "forward", "two_layer", 21),
    "forward_37x53_smooth_b3": (37, 53, 3, "forward", "smooth", 22),
    "backward_130x98_smooth_b3": (130, 98, 3, "backward", "smooth", 23),
    "backward_64x80_holes": (64, 80, 1, "backward", "holes", 101),
    "lateral_130x98_two_layer_b3": (130, 98, 3, "lateral", "two_layer", 31),
    "rotation_64x80_smooth_b3": (64, 80, 3, "rotation", "smooth", 102),
    "rotation_37x53_holes": (37, 53, 1, "rotation", "holes", 106),
    "rotation_256x320_two_layer_b3": (256, 320, 3, "rotation", "two_layer", 43),
    "behind_256x320_b3": (256, 320, 3, "behind", "near_far", 51),
    "behind_37x53": (37, 53, 1, "behind", "near_far", 52),
    "outside_64x80_smooth_b3": (64, 80, 3, "outside", "smooth", 61),
    "tiny_2x2": (2, 2, 1, "small", "smooth", 71),
    "tiny_2x2_b3": (2, 2, 3, "small", "smooth", 72),
    "tiny_3x5": (3, 5, 1, "small", "smooth", 73),
    "tiny_3x5_b3": (3, 5, 3, "small", "smooth", 74),
}
TWO_LAYER_CASES = sorted(n for n, c in SPLAT_CASES.items() if c[4] == "two_layer")


def min_landing(name):
    """Every case has a fifth of its points landing inside the target, except the one whose motion sends most of them outside."""
    return 0.02 if SPLAT_CASES[name][3] == "outside" else MIN_LANDING


def translation(tx, ty, tz):
    M = np.eye(4)
    M[:3, 3] = (tx, ty, tz)
    return M


def rotation_y(degrees):
    a = math.radians(degrees)
    M = np.eye(4)
    M[0, 0], M[0, 2], M[2, 0], M[2, 2] = math.cos(a), math.sin(a), -math.sin(a), math.cos(a)
    return M


def _motion(kind, rng):
    """-> (4x4 float64 transformation, scale of the half-resolution focal lengths)."""
    if kind == "scene":                                     # sample-scene pose pairs 1 to 11 frames apart
        poses = syn.sample_poses()
        a = int(rng.randint(12, len(poses)))
        return np.linalg.inv(poses[a]) @ poses[a - int(rng.randint(1, 12))], 1.0
    if kind == "forward":                                   # towards the scene: magnification
        return translation(0.0, 0.0, -rng.uniform(0.3, 0.45)), 1.0
    if kind == "backward":                                  # away from it: minification, many source points per cell
        return translation(0.0, 0.0, rng.uniform(0.2, 0.3)), 1.0
    if kind == "lateral":                                   # parallax: the foreground slides over the wall
        return translation(rng.choice([-1, 1]) * rng.uniform(0.2, 0.3), rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05)), 1.0
    if kind == "rotation":     # 20 to 40 degrees about y, another focal length in the target (a small step along z: a zero depth then has z != 0)
        return rotation_y(rng.choice([-1, 1]) * rng.uniform(20.0, 40.0)) @ translation(0.0, rng.uniform(-0.05, 0.05), rng.uniform(0.03, 0.08)), rng.uniform(0.7, 1.3)
    if kind == "behind":                                    # past the near surface: those points end up behind the camera
        return translation(rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), -rng.uniform(1.4, 1.6)), 1.0
    if kind == "outside":                                   # a long side step: most points leave the image
        return translation(rng.choice([-1, 1]) * rng.uniform(2.0, 2.4), rng.uniform(-0.1, 0.1), 0.0), 1.0
    if kind == "small":
        return translation(rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), rng.uniform(-0.05, 0.05)), 1.0
    raise KeyError(kind)


def _depth(kind, H, W, rng):
    """-> (depth [H,W] float64, near-layer mask [H,W] or None)."""
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    wave = lambda a, b: np.sin(a * xs / max(W, 8) + rng.uniform(0, 6)) * np.cos(b * ys / max(H, 8) + rng.uniform(0, 6))
    noise = lambda s: rng.uniform(-s, s, size=(H, W))
    smooth = 2.75 + 2.2 * wave(4.0, 3.0) + noise(0.03)                    # 0.5 to 5 m
    if kind == "smooth":
        return smooth, None
    if kind == "two_layer":                                 # a near foreground block over a far wall
        d = 4.0 + 0.4 * wave(3.0, 2.0) + noise(0.02)
        near = (ys >= H // 4) & (ys < (3 * H) // 4) & (xs >= W // 3) & (xs < (2 * W) // 3)
        d[near] = (1.2 + 0.1 * wave(5.0, 4.0) + noise(0.01))[near]
        return d, near
    if kind == "holes":                                     # blocks of 0 and of negative values, a few inf / nan pixels
        d = smooth
        d[H // 5:(2 * H) // 5, W // 6:W // 3] = 0.0
        d[(3 * H) // 5:(4 * H) // 5, W // 2:(3 * W) // 4] *= -1.0
        for n, value in enumerate((np.inf, np.nan, -np.inf, np.nan, np.inf)):
            d[(H * (2 * n + 1)) // 11, (W * (7 - n)) // 9] = value
        return d, None
    if kind == "near_far":                                  # more than a third of the image nearer than the camera's step
        d = 7.5 + 1.4 * wave(3.0, 2.0) + noise(0.03)
        near = xs < 0.38 * W
        d[near] = (0.75 + 0.2 * wave(4.0, 3.0) + noise(0.01))[near]
        return d, near
    raise KeyError(kind)


def splat_case(name):
    """-> dict(T [B,4,4], depth [B,1,H,W], full_K, half_K [B,3,3] float32 tensors, near [B,H,W] bool array or None).
    Every batch item has its own transformation and its own pair of intrinsics."""
    H, W, B, motion, kind, seed = SPLAT_CASES[name]
    rng = np.random.RandomState(seed)
    Ts, depths, fKs, hKs, nears = [], [], [], [], []
    for _ in range(B):
        M, focal = _motion(motion, rng)
        d, near = _depth(kind, H, W, rng)
        fx, fy = W * rng.uniform(0.85, 0.95), H * rng.uniform(1.05, 1.15)
        cx, cy = 0.5 * (W - 1) + W * rng.uniform(-0.03, 0.03), 0.5 * (H - 1) + H * rng.uniform(-0.03, 0.03)
        fK = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
        # half resolution: /2, the principal point off by a fraction of a pixel so that x / 2 does not sit on ties systematically
        hK = np.array([[0.5 * fx * focal, 0, 0.5 * cx + rng.uniform(-0.3, 0.3)], [0, 0.5 * fy * focal, 0.5 * cy + rng.uniform(-0.3, 0.3)], [0, 0, 1.0]])
        Ts.append(M), depths.append(d[None]), fKs.append(fK), hKs.append(hK), nears.append(near)
    t32 = lambda a: torch.from_numpy(np.stack(a).astype(np.float32))
    return dict(T=t32(Ts), depth=t32(depths), full_K=t32(fKs), half_K=t32(hKs), near=None if nears[0] is None else np.stack(nears))


# Cases whose arithmetic is exact in float32 and in float64 alike (powers of two and small dyadic numbers throughout, no rotation, z
# a power of two): the projected coordinates sit ON the ties n + 0.5 and on the borders -0.5, hw - 0.5, hh - 0.5 by construction, and
# nothing is ambiguous about them -- half to even decides, and the kernel's map equals ``SplatReference.exact`` bit for bit.
# name: (height, width, batch)
EXACT_CASES = {"ties_37x53_b3": (37, 53, 3), "ties_130x98": (130, 98, 1), "ties_8x12_b3": (8, 12, 3)}


def exact_case(name):
    H, W, B = EXACT_CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    Ts, depths, fKs, hKs = [], [], [], []
    for b in range(B):
        fx, fy = (64.0, 32.0, 128.0)[b % 3], (32.0, 64.0, 64.0)[b % 3]
        cx, cy = W // 2 + (0.0, 0.5, -1.0)[b % 3], H // 2 + (0.5, 0.0, 1.0)[b % 3]
        ratio = (0.5, 0.25, 0.5)[b % 3]                                  # half-resolution focal length / full-resolution one
        cxh, cyh = W // 4 + (0.0, 0.25, 0.5)[b % 3], H // 4 + (0.5, 0.0, 0.25)[b % 3]
        # u = (x - cx) * ratio + cxh + tx * fxh / d with d a power of two: multiples of 1 / 4, many of them n + 0.5
        tx, ty = (-1.0, 3.0, 2.0)[b % 3] / (fx * ratio), (1.0, -2.0, 3.0)[b % 3] / (fy * ratio)
        d = 2.0 ** rng.randint(-1, 3, size=(H, W))                      # 0.5, 1, 2, 4 m
        d[(ys % 7 == 3) & (xs % 5 == 1)] = 0.0
        d[(ys % 11 == 5) & (xs % 3 == 2)] *= -1.0
        Ts.append(translation(tx, ty, 0.0)), depths.append(d[None])
        fKs.append(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]]))
        hKs.append(np.array([[fx * ratio, 0, cxh], [0, fy * ratio, cyh], [0, 0, 1.0]]))
    t32 = lambda a: torch.from_numpy(np.stack(a).astype(np.float32))
    return dict(T=t32(Ts), depth=t32(depths), full_K=t32(fKs), half_K=t32(hKs))


def valid_factors(name):
    """The decimation factors that leave at least one row and one column of this case's half-resolution map."""
    H, W = (SPLAT_CASES[name] if name in SPLAT_CASES else EXACT_CASES[name])[:2]
    return [f for f in FACTORS if (H // 2) // f > 0 and (W // 2) // f > 0]


def layer_cells(ref, near):
    """Two-layer cases: (cells [B,hh,hw] on which certain points of BOTH layers land and no ambiguous one may, the far layer's
    largest z there, the near layer's largest z there)."""
    B, hh, hw = ref.shape
    far_z, near_z = np.zeros(B * hh * hw), np.zeros(B * hh * hw)
    sure = ref.lands & ~ref.ambiguous
    b = np.broadcast_to(np.arange(B)[:, None, None], sure.shape)
    lin = np.where(sure, (b * hh + ref.cell_i) * hw + ref.cell_j, 0).astype(np.int64)
    np.maximum.at(far_z, lin[sure & ~near], ref.z[sure & ~near])
    np.maximum.at(near_z, lin[sure & near], ref.z[sure & near])
    far_z, near_z = far_z.reshape(ref.shape), near_z.reshape(ref.shape)
    return (far_z > 0) & (near_z > 0) & ~ref.bracketed, far_z, near_z


# ---- TSDF integration ------------------------------------------------------------------------------------------------------------
def roundf(x, dtype):
    """C roundf: half away from zero."""
    return np.where(x >= 0, np.floor(x + dtype(0.5)), np.ceil(x - dtype(0.5))).astype(dtype)


def tsdf_integrate(tsdf_vol, weight_vol, color_vol, vol_origin, voxel_size, cam_intr, cam_pose, color_folded, depth_im, trunc_margin,
                   obs_weight=1.0, dtype=np.float32):
    """oracle/tsdf_oracle.py:integrate statement by statement, evaluated in ``dtype`` (the inputs are rounded to float32 first, as
    the kernel receives them).  In place; returns (mask of updated voxels, un-rounded pixel x, un-rounded pixel y, depth - cam_z)."""
    t = dtype
    X, Y, Z = tsdf_vol.shape
    im_h, im_w = depth_im.shape
    K, P = np.asarray(cam_intr, dtype=np.float32).astype(t), np.asarray(cam_pose, dtype=np.float32).astype(t)
    origin = np.asarray(vol_origin, dtype=np.float32).astype(t)
    vx, vy, vz = np.meshgrid(np.arange(X, dtype=t), np.arange(Y, dtype=t), np.arange(Z, dtype=t), indexing="ij")
    vs = t(np.float32(voxel_size))
    pt = [origin[0] + vx * vs, origin[1] + vy * vs, origin[2] + vz * vs]
    tmp = [pt[0] - P[0, 3], pt[1] - P[1, 3], pt[2] - P[2, 3]]
    cam = [P[0, k] * tmp[0] + P[1, k] * tmp[1] + P[2, k] * tmp[2] for k in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        raw_x = K[0, 0] * (cam[0] / cam[2]) + K[0, 2]
        raw_y = K[1, 1] * (cam[1] / cam[2]) + K[1, 2]
        px, py = roundf(raw_x, t), roundf(raw_y, t)
    ok = np.isfinite(px) & np.isfinite(py) & (px >= 0) & (px < im_w) & (py >= 0) & (py < im_h) & ~(cam[2] < 0)
    ix = np.where(ok, px, 0).astype(np.int64)
    iy = np.where(ok, py, 0).astype(np.int64)
    depth = np.asarray(depth_im, dtype=np.float32).astype(t)[iy, ix]
    ok &= depth != 0
    diff = depth - cam[2]
    tm = t(np.float32(trunc_margin))
    ok &= ~(diff < -tm)
    dist = np.minimum(t(1.0), diff / tm)
    w_old = weight_vol.copy()
    ow = t(np.float32(obs_weight))
    w_new = w_old + ow
    tsdf_new = (tsdf_vol * w_old + ow * dist) / w_new
    cc = t(65536.0)
    old = color_vol
    old_b = np.floor(old / cc)
    old_g = np.floor((old - old_b * cc) / t(256))
    old_r = old - old_b * cc - old_g * t(256)
    new = np.asarray(color_folded, dtype=np.float32).astype(t)[iy, ix]
    new_b = np.floor(new / cc)
    new_g = np.floor((new - new_b * cc) / t(256))
    new_r = new - new_b * cc - new_g * t(256)
    mix = lambda o, n: np.minimum(roundf((o * w_old + ow * n) / w_new, t), t(255.0))
    color_new = mix(old_b, new_b) * cc + mix(old_g, new_g) * t(256) + mix(old_r, new_r)
    weight_vol[ok] = w_new[ok]
    tsdf_vol[ok] = tsdf_new[ok].astype(t)
    color_vol[ok] = color_new[ok].astype(t)
    return ok, raw_x, raw_y, diff


def tsdf_explain(differs, vol_shape, vol_origin, voxel_size, frame, trunc_margin, delta=DELTA):
    """For the voxels of ``differs`` (kernel != float32 oracle after this frame): how many sit, in float64, within ``delta`` px of a
    roundf tie or within ``delta`` (relative to the margin) of the -trunc_margin edge.  The rest are the kernel's."""
    rgb, depth, K, pose, w = frame
    vols = [np.ones(vol_shape), np.zeros(vol_shape), np.zeros(vol_shape)]
    _, raw_x, raw_y, diff = tsdf_integrate(*vols, vol_origin, voxel_size, K, pose, np.zeros(depth.shape), depth, trunc_margin, w, np.float64)
    with np.errstate(invalid="ignore"):
        tie = (np.abs(raw_x - np.floor(raw_x) - 0.5) < delta) | (np.abs(raw_y - np.floor(raw_y) - 0.5) < delta)
        edge = np.abs(diff + trunc_margin) < delta * trunc_margin
    excused = differs & (tie | edge)
    return (f"{int(differs.sum())} voxels differ from the float32 oracle: {int((differs & tie).sum())} on a roundf tie, "
            f"{int((differs & edge & ~tie).sum())} on the truncation edge, {int((differs & ~excused).sum())} neither (kernel bug)")


# name: (dims, voxel size)
TSDF_VOLUMES = {"odd_37x53x29": ((37, 53, 29), 0.05), "grid_stride_200x150x160": ((200, 150, 160), 0.02)}
TSDF_WEIGHTS = (1.0, 2.5, 1.0, 0.5, 3.0, 1.0)


def tsdf_case(name):
    """-> (bounds [3,2], voxel size, six frames (rgb uint8 [H,W,3], depth float32 [H,W], K [3,3], camera-to-world pose [4,4], weight)).
    The camera orbits the volume's centre with rolled, rotated poses; frame 3 sits inside the volume and looks across it, so there
    are voxels behind it.  Depth images carry zero blocks and a step edge; every colour channel varies and reaches 0 and 255."""
    dims, voxel = TSDF_VOLUMES[name]
    dims = np.array(dims, dtype=np.float64)
    origin = np.array([-0.47, -0.31, 0.23])
    bounds = np.stack([origin, origin + (dims - 0.5) * voxel], axis=1)    # ceil((b1 - b0) / voxel) == dims, safely
    extent = dims * voxel
    centre = origin + 0.5 * extent
    H, W = 96, 128
    K = np.array([[110.3, 0.0, 63.37], [0.0, 108.7, 47.61], [0.0, 0.0, 1.0]])      # (no systematic projection ties)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    radius = 0.9 * extent.max()
    frames = []
    for n, w in enumerate(TSDF_WEIGHTS):
        azimuth, elevation, roll = math.radians(35.0 + 61.0 * n), math.radians((-20.0, 15.0, 40.0, 5.0, -35.0, 25.0)[n]), math.radians(17.0 * n - 30.0)
        direction = np.array([math.cos(elevation) * math.sin(azimuth), math.sin(elevation), math.cos(elevation) * math.cos(azimuth)])
        inside = n == 3
        position = centre + (0.15 * extent * direction if inside else radius * direction)
        forward = -direction                                               # look at (inside: across) the centre
        right = np.cross([0.0, 1.0, 0.0], forward)
        right /= np.linalg.norm(right)
        down = np.cross(forward, right)
        right, down = math.cos(roll) * right + math.sin(roll) * down, -math.sin(roll) * right + math.cos(roll) * down
        pose = np.eye(4)
        pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = right, down, forward, position
        reach = 0.4 * extent.min() if inside else radius
        depth = reach * (1.0 + 0.12 * np.sin(xs / 17.0 + n) + 0.08 * np.cos(ys / 13.0 - n))
        depth[:, (W * (3 + n)) // 10:] += 0.15 * extent.min()             # a step edge
        depth[10 + 5 * n:30 + 5 * n, 20 + 9 * n:50 + 9 * n] = 0.0        # invalid blocks
        depth[70:80, 100 - 11 * n:115 - 11 * n] = 0.0
        rgb = np.stack([(3 * xs + 7 * n) % 256, (255 - 2 * ys - 5 * n) % 256, (xs * ys + 90 + 31 * n) % 256], axis=-1)
        rgb[40:56, 30:60] = 255.0
        rgb[60:70, 64:100] = 0.0
        rgb[5:15, 90:120] = (255.0, 0.0, 255.0) if n % 2 else (0.0, 255.0, 0.0)
        frames.append((rgb.astype(np.uint8), depth.astype(np.float32), K.copy(), pose, w))
    return bounds, voxel, frames

"""Host definitions of the mesh rasteriser and of the vertex visibility (include/dvmvs_hip.h, "Mesh rasterisation"), and the scenes
their tests share.

``raster_fp32`` / ``visibility_fp32`` restate the definition operation by operation: ``np.float32`` scalars and arrays throughout (numpy
rounds every operation and fuses none), Python integers for the edge functions' coefficients and int64 arrays for their values.  The device
must reproduce them bit for bit.

``raster_f64`` is an independent reference: camera space, clipping (Sutherland-Hodgman against ``z >= near``), projection WITHOUT snapping
and the ray-plane depth in float64, the same top-left rule on the exact edge functions.  The fp32 definition differs from it in two ways,
which give the two bounds the comparison uses.

Edge band.  The fp32 definition moves each projected corner: by at most 1/512 px per axis from snapping to 8 sub-pixel bits (sqrt(2)/512 =
0.0028 px), and by the rounding of the fp32 projection.  The camera-space coordinates carry three products and three sums, each rounded:
at most 6 ulp of the largest term, 6 * 2^-24 * 8 m < 3e-6 m in the scenes below (|coordinates| < 8 m); a corner at depth z >= 1 m moves by
that times f / z <= 60 px/m, under 2e-4 px; the division, product and sum of ``(x / z) fx + cx`` add 3 ulp of at most 128 px, 2.3e-5 px.
In all under 0.0031 px.  A triangle whose corners each move by at most delta changes its coverage only within delta of its boundary
segments, so the two definitions can differ only at samples within 0.0031 px of a projected edge.  ``BAND`` = 1/128 px is 2.5 times that;
it excludes about 1-2 % of the pixels of the random scenes.

Depth tolerance.  The depth is not affected by snapping (the plane is that of the unsnapped triangle).  The perturbed corners (eps_p =
3e-6 m as above, scaled by the face's largest coordinate R / 8 m) move the plane, at a point inside the triangle, by at most eps_p along
the normal, which is eps_p * kappa along the ray, with kappa = |n| |d| / |n . d| (1 / cosine between ray and normal).  The cross product's
six products and three differences tilt the normal by at most 2^-22 * kappa_n, kappa_n = |e1| |e2| / |n|, which moves the depth at a point
at most rho (the longest edge) from corner a by rho * 2^-22 * kappa_n * kappa.  The remaining operations (two dot products of three terms,
the pixel's ray, one division) are relative: 8 ulp of z * kappa.  So
    tol = kappa * (6 * 2^-24 * R + 2^-22 * kappa_n * rho + 2^-21 * z)
per (pixel, face).  A pixel whose two nearest faces lie closer in depth than the sum of their tolerances may show either face and is
excluded, like a pixel in the band; everywhere else the faces must be equal and the depths within ``tol``.  At most ``MAX_EXCLUDED`` = 5 %
of the pixels may be excluded.
"""
import numpy as np

F32 = np.float32
BAND = 1.0 / 128.0
MAX_EXCLUDED = 0.05
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
SNAP_LIMIT = F32(2.0 ** 29)


def world_to_camera(cam_poses):
    """[N,3,4] float32 world-to-camera from camera-to-world [N,4,4]: the float64 inverse rounded once (the device layer computes its own
    in float64 too; the GPU tests hand the device's matrices to the restatement, so the two need not agree to the last bit)."""
    P = np.asarray(cam_poses, dtype=np.float64).reshape(-1, 4, 4)
    return np.linalg.inv(P)[:, :3, :].astype(np.float32)


def _camera_space(M, verts):
    x, y, z = verts[:, 0], verts[:, 1], verts[:, 2]
    return np.stack([((M[i, 0] * x + M[i, 1] * y) + M[i, 2] * z) + M[i, 3] for i in range(3)], axis=1)


def _clip(g, h, near):
    t = (near - g[2]) / (h[2] - g[2])
    return np.array([g[0] + t * (h[0] - g[0]), g[1] + t * (h[1] - g[1]), near], dtype=np.float32)


def _pieces_fp32(p, near):
    """Steps 3 of the definition: the corner lists of the pieces of the camera-space triangle p [3,3] (float32)."""
    behind = [bool(p[j, 2] < near) for j in range(3)]
    nb = sum(behind)
    if nb == 3:
        return []
    if nb == 0:
        return [[p[0], p[1], p[2]]]
    k = behind.index(True) if nb == 1 else behind.index(False)
    v0, v1, v2 = p[k], p[(k + 1) % 3], p[(k + 2) % 3]
    if nb == 1:
        q01, q02 = _clip(v0, v1, near), _clip(v0, v2, near)
        return [[q01, v1, v2], [q01, v2, q02]]
    return [[v0, _clip(v1, v0, near), _clip(v2, v0, near)]]


def _edge_setup(X, Y):
    """Step 5 with Python integers: [(a, b, c)] per edge with covered <=> a u + b v + c >= 0, or None for a piece without area."""
    area = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
    if area == 0:
        return None
    if area < 0:
        X, Y = [X[0], X[2], X[1]], [Y[0], Y[2], Y[1]]
    edges = []
    for i in range(3):
        j = (i + 1) % 3
        dx, dy = X[j] - X[i], Y[j] - Y[i]
        top_left = dy < 0 or (dy == 0 and dx > 0)
        edges.append((-dy * 256, dx * 256, dy * X[i] - dx * Y[i] - (0 if top_left else 1)))
    return edges


def raster_fp32(verts, faces, cam_intr, cam_w2c, height, width, near=0.05, far=np.inf, cull_backfaces=False):
    """The definition in float32: returns ``(depth [N,H,W] float32, face [N,H,W] int32, overflow [N] int32)``."""
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    K = np.asarray(cam_intr, dtype=np.float32).reshape(-1, 3, 3)
    M_all = np.asarray(cam_w2c, dtype=np.float32).reshape(-1, 3, 4)
    N, H, W, V = K.shape[0], int(height), int(width), verts.shape[0]
    near, far = F32(near), F32(far)
    keys = np.full((N, H, W), EMPTY, dtype=np.uint64)
    overflow = np.zeros(N, dtype=np.int32)
    with np.errstate(all="ignore"):
        for r in range(N):
            fx, fy, cx, cy = K[r, 0, 0], K[r, 1, 1], K[r, 0, 2], K[r, 1, 2]
            cam = _camera_space(M_all[r], verts)
            for f, (ia, ib, ic) in enumerate(faces):
                if min(ia, ib, ic) < 0 or max(ia, ib, ic) >= V:
                    continue
                p = cam[[ia, ib, ic]]
                if not np.all(np.isfinite(p)):
                    continue
                pieces = _pieces_fp32(p, near)
                if not pieces:
                    continue
                e1, e2 = p[1] - p[0], p[2] - p[0]
                nx = e1[1] * e2[2] - e1[2] * e2[1]
                ny = e1[2] * e2[0] - e1[0] * e2[2]
                nz = e1[0] * e2[1] - e1[1] * e2[0]
                na = (nx * p[0, 0] + ny * p[0, 1]) + nz * p[0, 2]
                if cull_backfaces and not na < 0:
                    continue
                lo = np.fmax(np.fmin(np.fmin(p[0, 2], p[1, 2]), p[2, 2]), near)
                hi = np.fmax(np.fmax(p[0, 2], p[1, 2]), p[2, 2])
                for piece in pieces:
                    X, Y, ok = [], [], True
                    for q in piece:
                        sx = np.rint(F32(256.0) * ((q[0] / q[2]) * fx + cx))
                        sy = np.rint(F32(256.0) * ((q[1] / q[2]) * fy + cy))
                        if not (abs(sx) <= SNAP_LIMIT and abs(sy) <= SNAP_LIMIT):
                            ok = False
                            break
                        X.append(int(sx))
                        Y.append(int(sy))
                    if not ok:
                        overflow[r] += 1
                        continue
                    edges = _edge_setup(X, Y)
                    if edges is None:
                        continue
                    u0, u1 = max((min(X) + 255) >> 8, 0), min(max(X) >> 8, W - 1)
                    v0, v1 = max((min(Y) + 255) >> 8, 0), min(max(Y) >> 8, H - 1)
                    if u0 > u1 or v0 > v1:
                        continue
                    vv, uu = np.meshgrid(np.arange(v0, v1 + 1, dtype=np.int64), np.arange(u0, u1 + 1, dtype=np.int64), indexing="ij")
                    covered = np.ones(uu.shape, dtype=bool)
                    for a, b, c in edges:
                        covered &= (a * uu + b * vv + c) >= 0
                    if not covered.any():
                        continue
                    dx = (uu.astype(np.float32) - cx) / fx
                    dy = (vv.astype(np.float32) - cy) / fy
                    den = (nx * dx + ny * dy) + nz
                    z = np.fmin(np.fmax(na / den, lo), hi).astype(np.float32)
                    covered &= ~(z > far)
                    key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
                    tile = keys[r, v0:v1 + 1, u0:u1 + 1]
                    tile[covered] = np.minimum(tile[covered], key[covered])
    hit = keys != EMPTY
    depth = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), F32(0.0)).astype(np.float32)
    face = np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    return depth, face, overflow


def visibility_fp32(verts, depth, cam_intr, cam_w2c, near=0.05, relative=0.01, absolute=0.0):
    """The vertex visibility of the definition in float32: int32 [V]."""
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    depth = np.asarray(depth, dtype=np.float32)
    K = np.asarray(cam_intr, dtype=np.float32).reshape(-1, 3, 3)
    M_all = np.asarray(cam_w2c, dtype=np.float32).reshape(-1, 3, 4)
    N, H, W = depth.shape
    near, scale, absolute = F32(near), F32(1.0) + F32(relative), F32(absolute)
    count = np.zeros(verts.shape[0], dtype=np.int32)
    with np.errstate(all="ignore"):
        for r in range(N):
            fx, fy, cx, cy = K[r, 0, 0], K[r, 1, 1], K[r, 0, 2], K[r, 1, 2]
            p = _camera_space(M_all[r], verts)
            z = p[:, 2]
            xp, yp = (p[:, 0] / z) * fx + cx, (p[:, 1] / z) * fy + cy
            ok = (z >= near) & (xp >= 0) & (xp <= F32(W - 1)) & (yp >= 0) & (yp <= F32(H - 1))
            x0 = np.where(ok, np.floor(xp), 0).astype(np.int64)
            y0 = np.where(ok, np.floor(yp), 0).astype(np.int64)
            best = np.zeros(verts.shape[0], dtype=np.float32)
            for dy in (0, 1):
                for dx in (0, 1):
                    inside = ok & (x0 + dx < W) & (y0 + dy < H)
                    d = depth[r, np.minimum(y0 + dy, H - 1), np.minimum(x0 + dx, W - 1)]
                    better = inside & (d > best)
                    best = np.where(better, d, best)
            count += (ok & (best > 0) & (z <= best * scale + absolute)).astype(np.int32)
    return count


def kept_faces(faces, count, min_views=1):
    """The faces whose three vertices are each seen by at least ``min_views`` views (what ``dvmvs.tsdf.visible_mesh`` keeps)."""
    faces = np.asarray(faces)
    return faces[(np.asarray(count)[faces] >= min_views).all(axis=1)]


# ----------------------------------------------------------------------------------------------------------------------
# the float64 reference
# ----------------------------------------------------------------------------------------------------------------------
def _clip_polygon_f64(poly, near):
    out = []
    for i in range(len(poly)):
        a, b = poly[i], poly[(i + 1) % len(poly)]
        ain, bin_ = a[2] >= near, b[2] >= near
        if ain:
            out.append(a)
        if ain != bin_:
            g, h = (a, b) if not ain else (b, a)
            t = (near - g[2]) / (h[2] - g[2])
            q = g + t * (h - g)
            q[2] = near
            out.append(q)
    return out


def raster_f64(verts, faces, cam_intr, cam_w2c, height, width, near=0.05, far=np.inf):
    """The float64 reference.  Returns a dict of [N,H,W] arrays: ``depth`` (0 = nothing) and ``face`` (-1) of the nearest face, ``tol`` (its
    depth tolerance, module docstring), ``ambiguous`` (the second nearest face lies within the sum of the two tolerances) and ``band``
    (the sample is within ``BAND`` pixels of a projected edge of some face)."""
    verts = np.asarray(verts, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    K = np.asarray(cam_intr, dtype=np.float32).astype(np.float64).reshape(-1, 3, 3)
    M_all = np.asarray(cam_w2c, dtype=np.float32).astype(np.float64).reshape(-1, 3, 4)
    N, H, W = K.shape[0], int(height), int(width)
    z1 = np.full((N, H, W), np.inf)
    z2 = np.full((N, H, W), np.inf)
    t1 = np.zeros((N, H, W))
    t2 = np.zeros((N, H, W))
    f1 = np.full((N, H, W), -1, dtype=np.int32)
    band = np.zeros((N, H, W), dtype=bool)
    for r in range(N):
        fx, fy, cx, cy = K[r, 0, 0], K[r, 1, 1], K[r, 0, 2], K[r, 1, 2]
        cam = verts @ M_all[r, :, :3].T + M_all[r, :, 3]
        for f, idx in enumerate(faces):
            p = cam[idx]
            poly = _clip_polygon_f64([p[0].copy(), p[1].copy(), p[2].copy()], near)
            if len(poly) < 3:
                continue
            e1, e2 = p[1] - p[0], p[2] - p[0]
            n = np.cross(e1, e2)
            norm_n = np.linalg.norm(n)
            if norm_n == 0:
                continue
            na = n @ p[0]
            kappa_n = np.linalg.norm(e1) * np.linalg.norm(e2) / norm_n
            rho = max(np.linalg.norm(e1), np.linalg.norm(e2), np.linalg.norm(p[2] - p[1]))
            R = np.abs(p).max()
            lo, hi = max(p[:, 2].min(), near), p[:, 2].max()
            pts = np.array([[q[0] / q[2] * fx + cx, q[1] / q[2] * fy + cy] for q in poly])
            for k in range(1, len(poly) - 1):
                tri = pts[[0, k, k + 1]]
                area = (tri[1, 0] - tri[0, 0]) * (tri[2, 1] - tri[0, 1]) - (tri[1, 1] - tri[0, 1]) * (tri[2, 0] - tri[0, 0])
                if area == 0:
                    continue
                if area < 0:
                    tri = tri[[0, 2, 1]]
                u0, u1 = max(int(np.floor(tri[:, 0].min())) - 1, 0), min(int(np.ceil(tri[:, 0].max())) + 1, W - 1)
                v0, v1 = max(int(np.floor(tri[:, 1].min())) - 1, 0), min(int(np.ceil(tri[:, 1].max())) + 1, H - 1)
                if u0 > u1 or v0 > v1:
                    continue
                vv, uu = np.meshgrid(np.arange(v0, v1 + 1, dtype=np.float64), np.arange(u0, u1 + 1, dtype=np.float64), indexing="ij")
                covered = np.ones(uu.shape, dtype=bool)
                near_edge = np.zeros(uu.shape, dtype=bool)
                for i in range(3):
                    a, b = tri[i], tri[(i + 1) % 3]
                    dx, dy = b[0] - a[0], b[1] - a[1]
                    E = dx * (vv - a[1]) - dy * (uu - a[0])
                    top_left = dy < 0 or (dy == 0 and dx > 0)
                    covered &= (E > 0) | ((E == 0) & top_left)
                    length2 = dx * dx + dy * dy
                    s = np.clip(((uu - a[0]) * dx + (vv - a[1]) * dy) / length2, 0.0, 1.0) if length2 > 0 else np.zeros(uu.shape)
                    near_edge |= np.hypot(uu - (a[0] + s * dx), vv - (a[1] + s * dy)) < BAND
                band[r, v0:v1 + 1, u0:u1 + 1] |= near_edge
                if not covered.any():
                    continue
                d = np.stack([(uu - cx) / fx, (vv - cy) / fy, np.ones(uu.shape)], axis=-1)
                den = d @ n
                with np.errstate(all="ignore"):
                    z = np.clip(na / den, lo, hi)
                    kappa = norm_n * np.linalg.norm(d, axis=-1) / np.abs(den)
                tol = kappa * (6 * 2.0 ** -24 * R + 2.0 ** -22 * kappa_n * rho + 2.0 ** -21 * z)
                covered &= np.isfinite(z) & ~(z > far)
                vs, us = np.nonzero(covered)
                for y, x in zip(vs, us):
                    Y, X, zz, tt = v0 + y, u0 + x, z[y, x], tol[y, x]
                    if f1[r, Y, X] == f:
                        continue
                    if zz < z1[r, Y, X]:
                        z2[r, Y, X], t2[r, Y, X] = z1[r, Y, X], t1[r, Y, X]
                        z1[r, Y, X], t1[r, Y, X], f1[r, Y, X] = zz, tt, f
                    elif zz < z2[r, Y, X]:
                        z2[r, Y, X], t2[r, Y, X] = zz, tt
    hit = f1 >= 0
    second = np.where(np.isfinite(z2), z2, 0.0) - np.where(hit, z1, 0.0)
    return {"depth": np.where(hit, z1, 0.0), "face": f1, "tol": np.where(hit, t1, 0.0),
            "ambiguous": hit & np.isfinite(z2) & (second <= t1 + t2), "band": band}


def compare_with_f64(depth, face, ref):
    """The comparison rule of the module docstring: returns the excluded share of the pixels; raises AssertionError where a pixel that is
    not excluded differs in face or by more than its tolerance in depth."""
    excluded = ref["band"] | ref["ambiguous"]
    check = ~excluded
    assert np.array_equal(np.asarray(face)[check], ref["face"][check]), "faces differ outside the band"
    err = np.abs(np.asarray(depth, dtype=np.float64) - ref["depth"])
    worst = (err - ref["tol"])[check]
    assert worst.size == 0 or worst.max() <= 0, f"depth differs by {err[check].max():.3e} m, {worst.max():.3e} m over its tolerance"
    return float(excluded.mean())


# ----------------------------------------------------------------------------------------------------------------------
# scenes
# ----------------------------------------------------------------------------------------------------------------------
def intrinsics(f=60.0, cx=31.5, cy=23.5):
    return np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]], dtype=np.float32)


def look_at(eye, target, up=(0.0, -1.0, 0.0)):
    """Camera-to-world [4,4] float32 of a camera at ``eye`` looking at ``target`` (z forward, x right, y down)."""
    eye, target, up = (np.asarray(a, dtype=np.float64) for a in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(-up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    P = np.eye(4)
    P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = x, y, z, eye
    return P.astype(np.float32)


def views(n):
    """n camera-to-world poses near the origin looking down +z, slightly turned and shifted, with different intrinsics per view."""
    poses = [look_at((0.05 * i, -0.03 * i, 0.02 * i), (0.2 * i - 0.1, 0.1 * i, 3.0)) for i in range(n)]
    Ks = [intrinsics(60.0 + 7.0 * i, 31.5 + 1.25 * i, 23.5 - 0.75 * i) for i in range(n)]
    return np.stack(Ks), np.stack(poses)


def grid_mesh(seed=0, cells=(12, 16), height=48, width=64, K=None):
    """A jittered grid of ``cells`` (rows, columns) over a ``height`` x ``width`` image of camera ``K`` at the origin: 2 rows cols faces,
    each corner back-projected from its jittered pixel position at its own depth of 1-4 m."""
    rng = np.random.default_rng(seed)
    K = intrinsics() if K is None else K
    rows, cols = cells
    ys, xs = np.meshgrid(np.linspace(-2.0, height + 1.0, rows + 1), np.linspace(-2.0, width + 1.0, cols + 1), indexing="ij")
    xs = xs + rng.uniform(-0.4, 0.4, xs.shape) * (width / cols)
    ys = ys + rng.uniform(-0.4, 0.4, ys.shape) * (height / rows)
    z = rng.uniform(1.0, 4.0, xs.shape)
    verts = np.stack([(xs - K[0, 2]) / K[0, 0] * z, (ys - K[1, 2]) / K[1, 1] * z, z], axis=-1).reshape(-1, 3).astype(np.float32)
    index = np.arange((rows + 1) * (cols + 1)).reshape(rows + 1, cols + 1)
    a, b, c, d = index[:-1, :-1].ravel(), index[:-1, 1:].ravel(), index[1:, :-1].ravel(), index[1:, 1:].ravel()
    faces = np.concatenate([np.stack([a, b, c], axis=1), np.stack([b, d, c], axis=1)]).astype(np.int32)
    return verts, faces


def soup_mesh(seed=1, count=300, extent=8.0, height=48, width=64, K=None):
    """``count`` unconnected triangles of at most ``extent`` pixels, anywhere over (and a little beyond) the image, at 1-4 m."""
    rng = np.random.default_rng(seed)
    K = intrinsics() if K is None else K
    centre = np.stack([rng.uniform(-4.0, width + 4.0, count), rng.uniform(-4.0, height + 4.0, count)], axis=1)
    px = centre[:, None, :] + rng.uniform(-0.5 * extent, 0.5 * extent, (count, 3, 2))
    z = rng.uniform(1.0, 4.0, (count, 3))
    verts = np.stack([(px[..., 0] - K[0, 2]) / K[0, 0] * z, (px[..., 1] - K[1, 2]) / K[1, 1] * z, z], axis=-1).reshape(-1, 3).astype(np.float32)
    return verts, np.arange(3 * count, dtype=np.int32).reshape(count, 3)


def pixel_triangle(px, z, K=None):
    """One triangle with corners at the pixel positions ``px`` [3,2] and depth ``z`` (a fronto-parallel plane when one number) for a camera
    ``K`` at the origin.  With z a power of two and K's entries small integers or halves the projection is exact."""
    K = intrinsics(64.0, 32.0, 24.0) if K is None else K
    px = np.asarray(px, dtype=np.float64)
    z = np.broadcast_to(np.asarray(z, dtype=np.float64), (3,))
    verts = np.stack([(px[:, 0] - K[0, 2]) / K[0, 0] * z, (px[:, 1] - K[1, 2]) / K[1, 1] * z, z], axis=1).astype(np.float32)
    return verts, np.array([[0, 1, 2]], dtype=np.int32)


def box_mesh(lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0), inward=True):
    """A closed box of 12 triangles; ``inward``: the faces wind counter-clockwise seen from inside (a room)."""
    lo, hi = np.asarray(lo, dtype=np.float32), np.asarray(hi, dtype=np.float32)
    verts = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], dtype=np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]      # outward, counter-clockwise
    faces = []
    for a, b, c, d in quads:
        faces += [(a, b, c), (a, c, d)]
    faces = np.array(faces, dtype=np.int32)
    return verts, faces[:, ::-1].copy() if inward else faces


def wall(z, half=1.5, cells=6, x_offset=0.0):
    """A square wall of 2 cells^2 triangles in the plane of depth ``z``, facing the origin."""
    lin = np.linspace(-half, half, cells + 1)
    ys, xs = np.meshgrid(lin, lin + x_offset, indexing="ij")
    verts = np.stack([xs, ys, np.full(xs.shape, z)], axis=-1).reshape(-1, 3).astype(np.float32)
    index = np.arange((cells + 1) ** 2).reshape(cells + 1, cells + 1)
    a, b, c, d = index[:-1, :-1].ravel(), index[:-1, 1:].ravel(), index[1:, :-1].ravel(), index[1:, 1:].ravel()
    return verts, np.concatenate([np.stack([a, c, b], axis=1), np.stack([b, c, d], axis=1)]).astype(np.int32)


def room_mesh(half=1.0, cells=8):
    """The inside of the cube [-half, half]^3 as six walls of 2 cells^2 triangles each (vertices not shared between walls), and views from
    near its centre that face only the +z and the +x wall: (verts, faces, K [8,3,3], poses [8,4,4], 48, 64)."""
    lin = np.linspace(-half, half, cells + 1)
    a, b = (g.ravel() for g in np.meshgrid(lin, lin, indexing="ij"))
    index = np.arange((cells + 1) ** 2).reshape(cells + 1, cells + 1)
    i0, i1, i2, i3 = index[:-1, :-1].ravel(), index[:-1, 1:].ravel(), index[1:, :-1].ravel(), index[1:, 1:].ravel()
    quad = np.concatenate([np.stack([i0, i1, i2], axis=1), np.stack([i1, i3, i2], axis=1)])
    verts, faces = [], []
    for axis in range(3):
        for side in (-half, half):
            wall_verts = np.zeros((len(a), 3))
            wall_verts[:, axis], wall_verts[:, (axis + 1) % 3], wall_verts[:, (axis + 2) % 3] = side, a, b
            faces.append(quad + len(verts) * len(a))
            verts.append(wall_verts)
    targets = [(-0.3, 0.0, 1.0), (0.2, 0.1, 1.0), (0.6, -0.1, 1.0), (1.0, 0.0, 1.0), (1.0, 0.1, 0.6), (1.0, -0.1, 0.2), (1.0, 0.0, -0.3), (0.8, 0.2, 1.0)]
    poses = np.stack([look_at((0.1 * np.cos(i), 0.05 * np.sin(i), -0.1), t) for i, t in enumerate(targets)])
    K = np.repeat(intrinsics()[None], len(poses), axis=0)
    return np.concatenate(verts).astype(np.float32), np.concatenate(faces).astype(np.int32), K, poses, 48, 64


def two_walls():
    """A near wall at 2 m and a larger far wall at 4 m behind it, seen by one camera at the origin: the far wall's vertices behind the near
    wall are hidden, those beyond its rim are seen.  Returns (verts, faces, K [1,3,3], poses [1,4,4], H, W, number of near vertices)."""
    v_near, f_near = wall(2.0, half=0.6, cells=4)
    v_far, f_far = wall(4.0, half=3.0, cells=8)
    verts = np.concatenate([v_near, v_far])
    faces = np.concatenate([f_near, f_far + len(v_near)])
    return verts, faces, intrinsics()[None], np.eye(4, dtype=np.float32)[None], 48, 64, len(v_near)


# ----------------------------------------------------------------------------------------------------------------------
# the cases the CPU and the GPU tests share (each made once per process)
# ----------------------------------------------------------------------------------------------------------------------
def exact_camera():
    """K with f = 64, centre (32, 24) and the identity pose: with depths that are powers of two, pixel positions project exactly."""
    return intrinsics(64.0, 32.0, 24.0)[None], np.eye(4, dtype=np.float32)[None]


def fan_mesh():
    """The square [2,6]^2 (pixels, at 2 m) as four triangles around its centre: top, right, bottom, left.  Their twelve edges run in all
    eight directions, every diagonal in both."""
    px = np.array([[2, 2], [6, 2], [6, 6], [2, 6], [4, 4]], dtype=np.float64)
    K = intrinsics(64.0, 32.0, 24.0)
    verts = np.stack([(px[:, 0] - K[0, 2]) / K[0, 0] * 2.0, (px[:, 1] - K[1, 2]) / K[1, 1] * 2.0, np.full(5, 2.0)], axis=1).astype(np.float32)
    return verts, np.array([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]], dtype=np.int32)


FAN_PIXELS = {     # (u, v) per face, worked out by hand from the top-left rule
    0: [(2, 2), (3, 2), (4, 2), (5, 2), (3, 3), (4, 3)],
    1: [(5, 3), (4, 4), (5, 4), (5, 5)],
    2: [(3, 5), (4, 5)],
    3: [(2, 3), (2, 4), (3, 4), (2, 5)],
}


def floor_mesh():
    """A floor 0.5 m under the camera (y down) from z = -1 m to z = 3 m, 4 m wide, as two triangles: face 0 has two corners behind the
    camera, face 1 one.  A pixel (u, v) of the exact camera sees it at z = 32 / (v - 24) for v >= 35 (the far edge projects to v = 34.67)."""
    verts = np.array([[-2, 0.5, -1], [2, 0.5, -1], [2, 0.5, 3], [-2, 0.5, 3]], dtype=np.float32)
    return verts, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)


def hand_cases():
    """name -> (verts, faces, K [N,3,3], poses [N,4,4], H, W): the small scenes with known answers."""
    K, P = exact_camera()
    cases = {}
    cases["fan"] = fan_mesh() + (K, P, 48, 64)
    quad = pixel_triangle([[2, 2], [6, 2], [2, 6]], 2.0)[0], pixel_triangle([[6, 6], [2, 6], [6, 2]], 2.0)[0]
    cases["quad"] = (np.concatenate(quad), np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int32), K, P, 48, 64)
    cases["floor"] = floor_mesh() + (K, P, 48, 64)
    behind = pixel_triangle([[10, 10], [30, 10], [10, 30]], 2.0)[0] * np.float32(-1.0)
    cases["behind"] = (behind, np.array([[0, 1, 2]], dtype=np.int32), K, P, 48, 64)
    tri = pixel_triangle([[10, 10], [30, 12], [14, 33]], [2.0, 3.0, 2.5])[0]
    cases["duplicates"] = (np.concatenate([tri, tri, tri]), np.array([[6, 7, 8], [0, 1, 2], [3, 4, 5]], dtype=np.int32), K, P, 48, 64)
    far_out = np.array([[1.0e6, 0.0, 0.06], [0.0, 0.0, 2.0], [0.0, 1.0, 2.0]], dtype=np.float32)
    cases["overflow"] = (np.concatenate([far_out, tri]), np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int32), K, P, 48, 64)
    return cases


_cache = {}


def random_case(name):
    """"grid" or "soup": (verts, faces, K [1,3,3], poses [1,4,4], 48, 64), the camera at the origin."""
    if name not in _cache:
        mesh = grid_mesh() if name == "grid" else soup_mesh()
        _cache[name] = mesh + (intrinsics()[None], np.eye(4, dtype=np.float32)[None], 48, 64)
    return _cache[name]


def random_reference(name):
    """``raster_f64`` of ``random_case(name)`` (the identity pose inverts exactly, so it serves the host and the device alike)."""
    key = name + "/f64"
    if key not in _cache:
        verts, faces, K, P, H, W = random_case(name)
        _cache[key] = raster_f64(verts, faces, K, world_to_camera(P), H, W)
    return _cache[key]

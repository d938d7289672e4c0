"""Smoothing a triangle mesh: the umbrella Laplacian filter, Taubin's lambda / mu filter that does not shrink, and area-weighted vertex
normals from the faces: the step between a mesh that carries the depth noise of its volume at the scale of a voxel (``marching_cubes``,
``filter_components``) and ``simplify_mesh``, whose plane quadrics are exactly what that noise perturbs.

This module is the host definition, in numpy, importable without a GPU.  ``smooth_mesh_device`` and ``vertex_normals_device`` are the
same on the GPU (``dvmvs.hip.smooth``, csrc/mesh_smooth.hip) and give the same bits.

Arithmetic contract (include/dvmvs_hip.h states it for the C entries): float64 computed from the float32 inputs with +, -, *, / and sqrt
only, every operation correctly rounded, nothing fused.  With V vertices and F faces (2^28 of each at most):

1. FACES THAT COUNT.  A face counts when its three indices lie in [0, V) and are pairwise different.  Every other face takes no part in
   rows, boundary or normals; it still comes back unchanged in ``faces``.
2. ROWS.  ``N(v)`` is the set of distinct u that share a counting face with v, in ascending u.  A counting face (a, b, c) emits the six
   directed pairs (a,b), (b,a), (b,c), (c,b), (c,a), (a,c): every edge once each way.  ``boundary[v]`` is true when some pair (v, u) is
   emitted exactly once over all counting faces: an edge of one face is boundary; an edge of two faces is not, whatever their
   orientation; an edge of three faces is not.
3. A STEP with factor s (a Python float, taken as float64); all reads come from the previous iterate.  If ``n = |N(v)|`` is 0, or the
   boundary is ``"fixed"`` and ``boundary[v]``, the position's bits are copied.  Otherwise, per component,
   ``S = (((0.0 + x_u1) + x_u2) + ...)`` over N(v) in order, ``m = S / float64(n)`` and ``x' = float32(x_v + s * (m - x_v))``.  The
   iterate between steps is float32.
4. METHODS.  ``"laplacian"``: one step with ``lam`` per iteration.  ``"taubin"``: a step with ``lam``, then a step with ``mu``, per
   iteration.  ``iterations == 0`` moves nothing.
5. VERTEX NORMALS (``vertex_normals`` always; ``smooth_mesh`` when ``recompute_normals`` is true and ``normals`` is given).  The sum for a
   vertex runs over its incidences (f, j): the counting faces f whose corner j is the vertex, in ascending ``3 f + j``.  Each contributes
   ``n_f = e1 x e2`` with ``e1 = p1 - p0``, ``e2 = p2 - p0`` of the FINAL float32 positions taken as float64,
   ``n_f = (e1_y e2_z - e1_z e2_y, e1_z e2_x - e1_x e2_z, e1_x e2_y - e1_y e2_x)``: area-weighted, not normalised per face.  The three
   sums start from 0.0; ``len = sqrt((x x + y y) + z z)``; each component is divided by ``len`` and rounded to float32.  Unless
   ``0 < len < inf`` the result is the fallback normal's bits (the input ``normals``), or (0, 0, 0) where there is none.  The meshes of
   this package wind counter-clockwise seen from the side their normals point to, so these normals agree with the ones they replace.
   With ``recompute_normals=False`` the input normals come back unchanged.

Coordinates that are not finite are outside the contract: the result is unspecified, but nothing is addressed out of bounds.
"""
import math
from typing import NamedTuple

import numpy as np

from dvmvs.simplify import _run_sums

MAX_ELEMENTS = 1 << 28               # vertices and faces the kernels take
MAX_ITERATIONS = 1024
METHODS = ("taubin", "laplacian")
BOUNDARIES = ("free", "fixed")


class SmoothSettings(NamedTuple):
    """How ``smooth_mesh`` smooths: the number of iterations, the method (``"taubin"``: a step with ``lam`` then one with ``mu`` per
    iteration; ``"laplacian"``: a step with ``lam``), the two factors, whether boundary vertices move (``"free"``) or keep their bits
    (``"fixed"``), and whether given normals are recomputed from the smoothed faces."""
    iterations: int
    method: str = "taubin"
    lam: float = 0.5
    mu: float = -0.53
    boundary: str = "free"
    recompute_normals: bool = True


def smooth_settings(settings):
    """The fields of a ``SmoothSettings`` as ``(int, str, float, float, str, bool)``; ``ValueError`` for anything else: iterations that are
    no int in [0, 1024], a ``lam`` outside (0, 1], for Taubin a ``mu`` outside [-1, -lam), an unknown method or boundary, a number that is
    not finite."""
    if not isinstance(settings, SmoothSettings):
        raise ValueError(f"expected a SmoothSettings, got {type(settings).__name__}")
    return _settings(*settings)


def _number(value):
    return not isinstance(value, bool) and isinstance(value, (int, float, np.integer, np.floating))


def _settings(iterations, method, lam, mu, boundary, recompute_normals):
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or not 0 <= int(iterations) <= MAX_ITERATIONS:
        raise ValueError(f"smooth_mesh: iterations must be an int in [0, {MAX_ITERATIONS}], got {iterations!r}")
    if not isinstance(method, str) or method not in METHODS:
        raise ValueError(f"smooth_mesh: method must be one of {METHODS}, got {method!r}")
    if not isinstance(boundary, str) or boundary not in BOUNDARIES:
        raise ValueError(f"smooth_mesh: boundary must be one of {BOUNDARIES}, got {boundary!r}")
    if not _number(lam) or not math.isfinite(float(lam)) or not 0.0 < float(lam) <= 1.0:
        raise ValueError(f"smooth_mesh: lam must be a finite number in (0, 1], got {lam!r}")
    if not _number(mu) or not math.isfinite(float(mu)):
        raise ValueError(f"smooth_mesh: mu must be a finite number, got {mu!r}")
    if method == "taubin" and not -1.0 <= float(mu) < -float(lam):
        raise ValueError(f"smooth_mesh: Taubin's mu must lie in [-1, -lam) = [-1, {-float(lam)}), got {mu!r}")
    if not isinstance(recompute_normals, (bool, np.bool_)):
        raise ValueError(f"smooth_mesh: recompute_normals must be a bool, got {recompute_normals!r}")
    return int(iterations), str(method), float(lam), float(mu), str(boundary), bool(recompute_normals)


def step_factors(iterations, method, lam, mu):
    """The factors of the steps of checked settings, in order: ``lam`` per iteration, for Taubin ``lam`` then ``mu``."""
    return [lam, mu] * iterations if method == "taubin" else [lam] * iterations


def _mesh(verts, faces, name="smooth_mesh"):
    verts = np.ascontiguousarray(verts, dtype=np.float32)
    if verts.ndim != 2 or verts.shape[1] != 3:
        raise ValueError(f"verts must be float32 [V,3], got {verts.shape}")
    faces = np.ascontiguousarray(faces, dtype=np.int32)
    if faces.ndim != 2 or faces.shape[1] != 3:
        raise ValueError(f"faces must be int32 [F,3], got {faces.shape}")
    if len(verts) > MAX_ELEMENTS or len(faces) > MAX_ELEMENTS:
        raise ValueError(f"{name}: {len(verts)} vertices and {len(faces)} faces are outside what is taken (2^28 at most)")
    return verts, faces


def _arguments(verts, faces, iterations, normals, colors, method, lam, mu, boundary, recompute_normals):
    if isinstance(iterations, SmoothSettings):
        iterations, method, lam, mu, boundary, recompute_normals = iterations
    settings = _settings(iterations, method, lam, mu, boundary, recompute_normals)
    verts, faces = _mesh(verts, faces)
    V = len(verts)
    if normals is not None:
        normals = np.ascontiguousarray(normals, dtype=np.float32)
        if normals.shape != verts.shape:
            raise ValueError(f"normals must be float32 [{V},3], got {normals.shape}")
    if colors is not None:
        colors = np.ascontiguousarray(colors, dtype=np.uint8)
        if colors.shape != verts.shape:
            raise ValueError(f"colors must be uint8 [{V},3], got {colors.shape}")
    return (verts, faces, normals, colors) + settings


def _counting(faces, V):
    """bool [F]: step 1."""
    a, b, c = faces[:, 0], faces[:, 1], faces[:, 2]
    return np.all((faces >= 0) & (faces < V), axis=1) & (a != b) & (b != c) & (a != c)


def _rows(faces, V):
    good = faces[_counting(faces, V)].astype(np.int64)
    a, b, c = good[:, 0], good[:, 1], good[:, 2]
    first = np.stack([a, b, b, c, c, a], axis=1).reshape(-1)
    second = np.stack([b, a, c, b, a, c], axis=1).reshape(-1)
    keys, times = np.unique((first << 32) | second, return_counts=True)
    owner = keys >> 32
    offsets = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=V))]).astype(np.int64)
    boundary = np.zeros(V, dtype=bool)
    boundary[owner[times == 1]] = True
    return offsets, (keys & 0xffffffff).astype(np.int32), boundary


def vertex_rows(faces, V):
    """``(offsets int64 [V+1], neighbours int32 [E], boundary bool [V])``: step 2.  ``neighbours[offsets[v]:offsets[v+1]]`` is N(v)."""
    if isinstance(V, bool) or not isinstance(V, (int, np.integer)) or not 0 <= int(V) <= MAX_ELEMENTS:
        raise ValueError(f"vertex_rows: V must be a number of vertices in [0, 2^28], got {V!r}")
    _, faces = _mesh(np.zeros((0, 3), np.float32), faces, "vertex_rows")
    return _rows(faces, int(V))


def _step(x32, offsets, neighbours, frozen, s):
    """Step 3 on all vertices at once."""
    counts = np.diff(offsets)
    x = x32.astype(np.float64)
    with np.errstate(all="ignore"):
        sums = _run_sums(x[neighbours], offsets[:-1], counts)
        moves = (counts > 0) & ~frozen
        mean = sums / np.where(moves, counts, 1).astype(np.float64)[:, None]
        new = (x + s * (mean - x)).astype(np.float32)
    return np.where(moves[:, None], new, x32)


def _normals(verts, faces, fallback):
    """Step 5."""
    V = len(verts)
    counting = _counting(faces, V)
    good = faces[counting].astype(np.int64)
    ids = (3 * np.flatnonzero(counting)[:, None] + np.arange(3)[None, :]).reshape(-1)          # 3 f + j, ascending
    owner = good.reshape(-1)
    order = np.argsort(owner, kind="stable")
    owner, ids = owner[order], ids[order]
    counts = np.bincount(owner, minlength=V).astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    tri = faces[ids // 3].astype(np.int64)
    v64 = verts.astype(np.float64)
    with np.errstate(all="ignore"):
        e1, e2 = v64[tri[:, 1]] - v64[tri[:, 0]], v64[tri[:, 2]] - v64[tri[:, 0]]
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1).reshape(-1, 3)
        s = _run_sums(n, starts, counts)
        length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        ok = (length > 0.0) & (length < np.inf)
        unit = (s / np.where(ok, length, 1.0)[:, None]).astype(np.float32)
    return np.where(ok[:, None], unit, np.zeros((V, 3), np.float32) if fallback is None else fallback)


def vertex_normals(verts, faces, fallback=None):
    """float32 [V,3]: the area-weighted vertex normals of the mesh by step 5; where a vertex has none (no counting face, or faces
    without area) the row of ``fallback`` float32 [V,3], or zeros."""
    verts, faces = _mesh(verts, faces, "vertex_normals")
    if fallback is not None:
        fallback = np.ascontiguousarray(fallback, dtype=np.float32)
        if fallback.shape != verts.shape:
            raise ValueError(f"fallback must be float32 [{len(verts)},3], got {fallback.shape}")
    return _normals(verts, faces, fallback)


def smooth_mesh(verts, faces, iterations, normals=None, colors=None, method="taubin", lam=0.5, mu=-0.53, boundary="free",
                recompute_normals=True):
    """The mesh ``verts`` float32 [V,3], ``faces`` int32 [F,3] after ``iterations`` of the filter ``method`` by the module's definition:
    ``(verts', faces, normals' or None, colors or None)``, the 4-tuple of ``simplify_mesh``, so the stages chain.  ``faces`` and
    ``colors`` uint8 [V,3] come back unchanged, as copies; ``normals`` float32 [V,3] are recomputed from the smoothed faces
    (``recompute_normals``) or come back unchanged; V and F never change.  A ``SmoothSettings`` in place of ``iterations`` brings the
    rest.  Raises ``ValueError`` for settings that ``smooth_settings`` refuses."""
    verts, faces, normals, colors, iterations, method, lam, mu, boundary, recompute_normals = _arguments(
        verts, faces, iterations, normals, colors, method, lam, mu, boundary, recompute_normals)
    offsets, neighbours, on_boundary = _rows(faces, len(verts))
    frozen = on_boundary if boundary == "fixed" else np.zeros(len(verts), dtype=bool)
    position = verts.copy()
    for s in step_factors(iterations, method, lam, mu):
        position = _step(position, offsets, neighbours, frozen, s)
    if normals is not None:
        normals = _normals(position, faces, normals) if recompute_normals else normals.copy()
    return position, faces.copy(), normals, None if colors is None else colors.copy()


def _smooth_scalar(verts, faces, iterations, normals=None, colors=None, method="taubin", lam=0.5, mu=-0.53, boundary="free",
                   recompute_normals=True):
    """``smooth_mesh`` as a loop over the vertices in Python floats (IEEE float64, every operation rounded on its own): the definition read
    line by line.  Slow; the tests hold ``smooth_mesh`` equal to it bit for bit."""
    verts, faces, normals, colors, iterations, method, lam, mu, boundary, recompute_normals = _arguments(
        verts, faces, iterations, normals, colors, method, lam, mu, boundary, recompute_normals)
    V, F = len(verts), len(faces)
    counting, pairs = [], {}
    for f in range(F):
        a, b, c = (int(t) for t in faces[f])
        if not (0 <= a < V and 0 <= b < V and 0 <= c < V) or a == b or b == c or a == c:
            continue
        counting.append(f)
        for pair in ((a, b), (b, a), (b, c), (c, b), (c, a), (a, c)):
            pairs[pair] = pairs.get(pair, 0) + 1
    rows = [[] for _ in range(V)]
    on_boundary = [False] * V
    for (a, b) in sorted(pairs):                                   # ascending u within every row
        rows[a].append(b)
        if pairs[(a, b)] == 1:
            on_boundary[a] = True
    position = verts.copy()
    for s in step_factors(iterations, method, lam, mu):
        new = position.copy()
        for v in range(V):
            n = len(rows[v])
            if n == 0 or (boundary == "fixed" and on_boundary[v]):
                continue
            for k in range(3):
                total = 0.0
                for u in rows[v]:
                    total = total + float(position[u][k])
                x = float(position[v][k])
                new[v][k] = _f32(x + s * (_div(total, float(n)) - x))
        position = new
    if normals is not None and recompute_normals:
        sums = [[0.0, 0.0, 0.0] for _ in range(V)]
        for f in counting:                                           # ascending 3 f + j for every vertex
            p = [[float(position[int(faces[f][k])][a]) for a in range(3)] for k in range(3)]
            e1 = [p[1][a] - p[0][a] for a in range(3)]
            e2 = [p[2][a] - p[0][a] for a in range(3)]
            n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
            for j in range(3):
                t = sums[int(faces[f][j])]
                for k in range(3):
                    t[k] = t[k] + n[k]
        new_normals = normals.copy()
        for v in range(V):
            t = sums[v]
            sq = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]
            length = math.sqrt(sq) if sq >= 0.0 else math.nan
            if 0.0 < length < math.inf:
                new_normals[v] = [_f32(_div(t[k], length)) for k in range(3)]
        normals = new_normals
    elif normals is not None:
        normals = normals.copy()
    return position, faces.copy(), normals, None if colors is None else colors.copy()


def _f32(x):
    """x rounded to float32 without a warning where it overflows."""
    with np.errstate(all="ignore"):
        return np.float64(x).astype(np.float32)


def _div(a, b):
    """a / b in float64 as IEEE has it where Python would raise."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def smooth_mesh_device(verts, faces, iterations, normals=None, colors=None, method="taubin", lam=0.5, mu=-0.53, boundary="free",
                       recompute_normals=True):
    """``smooth_mesh`` for device tensors (``dvmvs.hip.smooth.smooth_mesh``): the same bits, on the GPU."""
    from dvmvs.hip import smooth
    return smooth.smooth_mesh(verts, faces, iterations, normals, colors, method, lam, mu, boundary, recompute_normals)


def vertex_normals_device(verts, faces, fallback=None):
    """``vertex_normals`` for device tensors (``dvmvs.hip.smooth.vertex_normals``): the same bits, on the GPU."""
    from dvmvs.hip import smooth
    return smooth.vertex_normals(verts, faces, fallback)

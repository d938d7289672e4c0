"""Simplifying a triangle mesh by vertex clustering with quadric error representatives (Lindstrom 2000): the step between a mesh that has
the density of its voxel grid and everything that stores, views or scores it.  The vertices of a grid cell become one vertex, placed where
the summed plane quadrics of the faces around them are smallest, so that an edge or a corner of the surface stays an edge or a corner and
a flat wall stays in its plane; a cell mean would round both off by a fraction of the cell.

This module is the host definition, in numpy, importable without a GPU.  ``simplify_mesh_device`` is the same on the GPU
(``dvmvs.hip.simplify``, csrc/mesh_simplify.hip) and gives the same bits.

Arithmetic contract (include/dvmvs_hip.h states it for the C entries): float64 computed from the float32 inputs with +, -, *, / and sqrt
only, every operation correctly rounded, nothing fused.  With V vertices, F faces and the cell edge ``voxel``:

1. CLUSTERS are ``dvmvs.errors.voxel_down_sample``'s voxels of ``verts``: cell ``int((x - min) * float32(1 / voxel))`` per axis, key
   ``(cx << 42) | (cy << 21) | cz``, numbered in ascending key order; its errors are raised (a coordinate that is not finite, a cell index
   of 2^21 or more).  The cluster mean ``m_c`` is that function's point: the float64 sum over the members in ascending vertex index, one
   division, one rounding to float32.
2. The QUADRIC of cluster c runs over its incidences (f, j): face f has its three indices in [0, V) and corner j lies in c; in ascending
   ``3 f + j``.  A face with two corners in the cell counts twice, and a face that later degenerates still counts.  With
   ``o = float64(m_c)``, ``p_k = float64(verts[faces[f,k]]) - o``, ``e1 = p_1 - p_0``, ``e2 = p_2 - p_0``,
   ``n = (e1_y e2_z - e1_z e2_y, e1_z e2_x - e1_x e2_z, e1_x e2_y - e1_y e2_x)`` and ``d = -((n_x p_0x + n_y p_0y) + n_z p_0z)``:
   ``A_cd += n_c n_d`` for (c,d) = (0,0),(0,1),(0,2),(1,1),(1,2),(2,2) and ``b_c += d n_c``, all nine sums from 0.0.  (The area^2-weighted
   plane quadric about the cluster's own mean: the coordinates are small wherever the mesh lies.)
3. The REPRESENTATIVE.  ``contraction="average"``: ``m_c``.  Otherwise the cyclic Jacobi of ``dvmvs.normals`` on A (the same rotations, at
   most 16 sweeps, the same stop rule) gives ``l_0..2`` (the diagonal) and the columns ``v_0..2``.  ``l_max`` is ``l_0``, replaced by
   ``l_1`` when ``l_1 > l_max``, then by ``l_2`` likewise.  Column i is kept when ``l_i > 1e-3 * l_max``; x starts at (0, 0, 0) and for
   each kept column, in column order, ``x_k += (-(((v_0i b_0 + v_1i b_1) + v_2i b_2) / l_i)) * v_ki``.  When ``l_max > 0`` and
   ``|x_k| <= float64(float32(voxel))`` for every k (false for a NaN), the vertex is ``float32(o + x)``; otherwise it is ``m_c``.
4. ATTRIBUTES.  ``normals'``: the float64 sum of the members' normals in ascending vertex index, each component divided by
   ``len = sqrt((x x + y y) + z z)`` and rounded to float32; (0, 0, 0) unless ``0 < len < inf``.  ``colors'``: per channel
   ``rint(sum / n)`` of the members (the sum is an integer, exact in float64; halves go to even), as uint8.
5. FACES.  Each face is mapped to cluster numbers.  It is dropped when an index lies outside [0, V), when two of its mapped corners are
   equal, or when an earlier face (smaller index) has the same mapped corners up to rotation; the opposite orientation is another face and
   stays.  Survivors keep their order and their own corner order.
6. COMPACTION.  Clusters that no surviving face uses are removed, the others keep their order and are renumbered, the faces re-indexed.
"""
import math
from typing import NamedTuple

import numpy as np

from dvmvs.errors import voxel_down_sample, voxel_keys
from dvmvs.normals import _jacobi3

MAX_ELEMENTS = 1 << 28               # vertices and faces the kernels take
RANK_THRESHOLD = 1e-3                # a column of the Jacobi is kept when its eigenvalue exceeds this fraction of the largest
CONTRACTIONS = ("quadric", "average")
_SWEEPS = 16
_PAIRS = ((0, 1), (0, 2), (1, 2))
_UPPER = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


class SimplifySettings(NamedTuple):
    """How ``simplify_mesh`` simplifies: the edge of the clustering cells in metres, and where a cell's vertex goes: ``"quadric"`` (the
    minimiser of the summed plane quadrics) or ``"average"`` (the cell mean)."""
    voxel: float
    contraction: str = "quadric"


def simplify_settings(settings):
    """``(voxel, contraction)`` of a ``SimplifySettings`` as a float and a str; ``ValueError`` for anything else, a voxel that is not
    positive and finite, and a contraction that is not known."""
    if not isinstance(settings, SimplifySettings):
        raise ValueError(f"expected a SimplifySettings, got {type(settings).__name__}")
    return _settings(*settings)


def _settings(voxel, contraction):
    if isinstance(voxel, bool) or not isinstance(voxel, (int, float, np.integer, np.floating)):
        raise ValueError(f"simplify_mesh: voxel must be a number of metres, got {voxel!r}")
    voxel = float(voxel)
    if not voxel > 0.0 or voxel == np.inf:
        raise ValueError(f"simplify_mesh: voxel must be positive and finite, got {voxel}")
    if contraction not in CONTRACTIONS:
        raise ValueError(f"simplify_mesh: contraction must be one of {CONTRACTIONS}, got {contraction!r}")
    return voxel, str(contraction)


def _arguments(verts, faces, voxel, normals, colors, contraction):
    if isinstance(voxel, SimplifySettings):
        voxel, contraction = voxel
    voxel, contraction = _settings(voxel, contraction)
    verts = np.ascontiguousarray(verts, dtype=np.float32)
    if verts.ndim != 2 or verts.shape[1] != 3:
        raise ValueError(f"verts must be float32 [V,3], got {verts.shape}")
    faces = np.ascontiguousarray(faces, dtype=np.int32)
    if faces.ndim != 2 or faces.shape[1] != 3:
        raise ValueError(f"faces must be int32 [F,3], got {faces.shape}")
    V = len(verts)
    if V > MAX_ELEMENTS or len(faces) > MAX_ELEMENTS:
        raise ValueError(f"simplify_mesh: {V} vertices and {len(faces)} faces are outside what is taken (2^28 at most)")
    if normals is not None:
        normals = np.ascontiguousarray(normals, dtype=np.float32)
        if normals.shape != verts.shape:
            raise ValueError(f"normals must be float32 [{V},3], got {normals.shape}")
    if colors is not None:
        colors = np.ascontiguousarray(colors, dtype=np.uint8)
        if colors.shape != verts.shape:
            raise ValueError(f"colors must be uint8 [{V},3], got {colors.shape}")
    return verts, faces, voxel, normals, colors, contraction


def _empty(V, normals, colors, return_index):
    out = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), None if normals is None else np.zeros((0, 3), np.float32),
           None if colors is None else np.zeros((0, 3), np.uint8))
    return out + ((np.full(V, -1, np.int32), np.zeros(0, np.int32)),) if return_index else out


def _clusters(verts, voxel):
    """``(cluster int64 [V], order int64 [V], starts int64 [M], counts int64 [M], mean float32 [M,3])``: step 1."""
    keys, _, _ = voxel_keys(verts, voxel)
    order = np.argsort(keys, kind="stable")
    sorted_keys = keys[order]
    head = np.concatenate([[True], sorted_keys[1:] != sorted_keys[:-1]])
    starts = np.flatnonzero(head)
    counts = np.diff(np.concatenate([starts, [len(verts)]]))
    cluster = np.empty(len(verts), dtype=np.int64)
    cluster[order] = np.cumsum(head) - 1
    return cluster, order, starts, counts, voxel_down_sample(verts, voxel)


def _run_sums(values, starts, counts):
    """float64 [M, ...]: per run, the sum of ``values`` (float64, in run order) from 0.0 in ascending slot, vectorised over the runs: the
    r-th value of every run that has one is added in step r, as ``voxel_down_sample`` sums."""
    sums = np.zeros((len(starts),) + values.shape[1:], dtype=np.float64)
    if len(starts) == 0 or len(values) == 0:
        return sums
    by_count = np.argsort(-counts, kind="stable")
    descending = -counts[by_count]
    for r in range(int(counts.max())):
        active = by_count[:np.searchsorted(descending, -r, side="left")]
        sums[active] += values[starts[active] + r]
    return sums


def _quadrics(verts, faces, cluster, mean):
    """``(A float64 [M,6] in the order of _UPPER, b float64 [M,3])``: step 2."""
    V, M = len(verts), len(mean)
    valid = np.all((faces >= 0) & (faces < V), axis=1)
    good = faces[valid].astype(np.int64)
    ids = (3 * np.flatnonzero(valid)[:, None] + np.arange(3)[None, :]).reshape(-1)          # 3 f + j, ascending
    owner = cluster[good].reshape(-1)
    order = np.argsort(owner, kind="stable")
    owner, ids = owner[order], ids[order]
    counts = np.bincount(owner, minlength=M).astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    tri = faces[ids // 3].astype(np.int64)
    o = mean.astype(np.float64)[owner]
    v64 = verts.astype(np.float64)
    p0, p1, p2 = v64[tri[:, 0]] - o, v64[tri[:, 1]] - o, v64[tri[:, 2]] - o
    with np.errstate(all="ignore"):
        e1, e2 = p1 - p0, p2 - p0
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        d = -((n[:, 0] * p0[:, 0] + n[:, 1] * p0[:, 1]) + n[:, 2] * p0[:, 2])
        terms = np.stack([n[:, c] * n[:, e] for c, e in _UPPER] + [d * n[:, c] for c in range(3)], axis=1)
        sums = _run_sums(terms, starts, counts)
    return sums[:, :6], sums[:, 6:]


def _jacobi_columns(A6):
    """The cyclic Jacobi of ``dvmvs.normals.point_normals`` on M symmetric 3x3 at once: ``(diagonal [3] of float64 [M], V [3][3] of
    float64 [M])``."""
    M = len(A6)
    A = {cd: A6[:, k].copy() for k, cd in enumerate(_UPPER)}
    V = [[np.full(M, float(r == c)) for c in range(3)] for r in range(3)]
    for _ in range(_SWEEPS):
        if not ((A[(0, 1)] != 0.0) | (A[(0, 2)] != 0.0) | (A[(1, 2)] != 0.0)).any():
            break
        for p, q in _PAIRS:
            r = 3 - p - q
            pr, qr = (min(p, r), max(p, r)), (min(q, r), max(q, r))
            turn = A[(p, q)] != 0.0
            apq = np.where(turn, A[(p, q)], 1.0)
            theta = (A[(q, q)] - A[(p, p)]) / (2.0 * apq)
            t = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
            t = np.where(theta < 0.0, -t, t)
            c = 1.0 / np.sqrt(t * t + 1.0)
            sn = t * c
            app, aqq, apq = A[(p, p)], A[(q, q)], A[(p, q)]
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
    return [A[(0, 0)], A[(1, 1)], A[(2, 2)]], V


def _representatives(A6, b, mean, voxel):
    """``(position float32 [M,3], rank int32 [M])``: step 3 for the quadric contraction; rank = the kept columns (0 without a quadric)."""
    M = len(mean)
    with np.errstate(all="ignore"):
        lam, V = _jacobi_columns(A6)
        lmax = lam[0]
        lmax = np.where(lam[1] > lmax, lam[1], lmax)
        lmax = np.where(lam[2] > lmax, lam[2], lmax)
        threshold = RANK_THRESHOLD * lmax
        x = [np.zeros(M) for _ in range(3)]
        rank = np.zeros(M, dtype=np.int32)
        for i in range(3):
            kept = lam[i] > threshold
            dot = (V[0][i] * b[:, 0] + V[1][i] * b[:, 1]) + V[2][i] * b[:, 2]
            coef = -(dot / np.where(kept, lam[i], 1.0))
            for k in range(3):
                x[k] = np.where(kept, x[k] + coef * V[k][i], x[k])
            rank += kept
        limit = float(np.float32(voxel))
        moved = (lmax > 0.0) & (np.abs(x[0]) <= limit) & (np.abs(x[1]) <= limit) & (np.abs(x[2]) <= limit)
        o = mean.astype(np.float64)
        shifted = np.stack([o[:, k] + np.where(moved, x[k], 0.0) for k in range(3)], axis=1).astype(np.float32)
    return np.where(moved[:, None], shifted, mean), np.where(lmax > 0.0, rank, 0).astype(np.int32)


def quadric_ranks(verts, faces, voxel):
    """int32 [M]: for every cluster of step 1 (before the compaction) the number of columns that step 3 keeps: 1 on a plane, 2 on an
    edge, 3 at a corner, 0 for a cluster without a face of non-zero area."""
    verts, faces, voxel, _, _, _ = _arguments(verts, faces, voxel, None, None, "quadric")
    if len(verts) == 0:
        return np.zeros(0, np.int32)
    cluster, _, _, _, mean = _clusters(verts, voxel)
    A6, b = _quadrics(verts, faces, cluster, mean)
    return _representatives(A6, b, mean, voxel)[1]


def _attributes(normals, colors, order, starts, counts):
    """Step 4: ``(normals' float32 [M,3] or None, colors' uint8 [M,3] or None)`` of all clusters."""
    new_normals = new_colors = None
    if normals is not None:
        with np.errstate(all="ignore"):
            s = _run_sums(normals[order].astype(np.float64), starts, counts)
            length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
            ok = (length > 0.0) & (length < np.inf)
            new_normals = np.where(ok[:, None], s / np.where(ok, length, 1.0)[:, None], 0.0).astype(np.float32)
    if colors is not None:
        sums = np.add.reduceat(colors[order].astype(np.int64), starts, axis=0) if len(starts) else np.zeros((0, 3), np.int64)
        new_colors = np.rint(sums.astype(np.float64) / counts[:, None].astype(np.float64)).astype(np.uint8)
    return new_normals, new_colors


def _surviving_faces(faces, cluster, V):
    """Step 5: ``(mapped int64 [F,3] (rows of invalid faces undefined), keep bool [F])``."""
    F = len(faces)
    valid = np.all((faces >= 0) & (faces < V), axis=1)
    mapped = cluster[np.where(valid[:, None], faces, 0)] if V else np.zeros((F, 3), np.int64)
    a, b, c = mapped[:, 0], mapped[:, 1], mapped[:, 2]
    proper = valid & (a != b) & (b != c) & (a != c)
    # the rotation that puts the smallest corner first (the corners of a proper face are distinct)
    first_a, first_b = (a <= b) & (a <= c), (b <= a) & (b <= c)
    x = np.where(first_a, a, np.where(first_b, b, c))
    y = np.where(first_a, b, np.where(first_b, c, a))
    z = np.where(first_a, c, np.where(first_b, a, b))
    keep = np.zeros(F, dtype=bool)
    index = np.flatnonzero(proper)
    if len(index):
        order = index[np.lexsort((index, z[index], y[index], x[index]))]
        head = np.concatenate([[True], (x[order][1:] != x[order][:-1]) | (y[order][1:] != y[order][:-1]) | (z[order][1:] != z[order][:-1])])
        keep[order[head]] = True
    return mapped, keep


def _compact(position, new_normals, new_colors, mapped, keep, cluster, return_index):
    """Step 6."""
    M = len(position)
    face_index = np.flatnonzero(keep).astype(np.int32)
    used = np.zeros(M, dtype=bool)
    used[mapped[face_index].reshape(-1)] = True
    kept = np.flatnonzero(used)
    new_index = np.full(M, -1, dtype=np.int32)
    new_index[kept] = np.arange(len(kept), dtype=np.int32)
    new_faces = new_index[mapped[face_index]].reshape(-1, 3).astype(np.int32)
    out = (np.ascontiguousarray(position[kept], dtype=np.float32), new_faces, None if new_normals is None else new_normals[kept],
           None if new_colors is None else new_colors[kept])
    return out + ((new_index[cluster].astype(np.int32), face_index),) if return_index else out


def simplify_mesh(verts, faces, voxel, normals=None, colors=None, contraction="quadric", return_index=False):
    """The mesh ``verts`` float32 [V,3], ``faces`` int32 [F,3] with one vertex per occupied cell of edge ``voxel`` metres, by the module's
    definition: ``(verts', faces', normals' or None, colors' or None)``; ``normals`` float32 [V,3] and ``colors`` uint8 [V,3] are merged
    alongside.  ``contraction``: ``"quadric"`` or ``"average"``; a ``SimplifySettings`` in place of ``voxel`` brings both.  With
    ``return_index`` also ``(vertex_cluster int32 [V], face_index int32 [F'])``: the output vertex that vertex i became (-1 where its
    cluster kept no face) and the old index of every output face.  Raises ``ValueError`` for a voxel that is not positive and finite and
    where ``voxel_down_sample`` does (a coordinate that is not finite, a cell index of 2^21 or more)."""
    verts, faces, voxel, normals, colors, contraction = _arguments(verts, faces, voxel, normals, colors, contraction)
    V = len(verts)
    if V == 0:
        return _empty(V, normals, colors, return_index)
    cluster, order, starts, counts, mean = _clusters(verts, voxel)
    if contraction == "quadric":
        A6, b = _quadrics(verts, faces, cluster, mean)
        position, _ = _representatives(A6, b, mean, voxel)
    else:
        position = mean
    new_normals, new_colors = _attributes(normals, colors, order, starts, counts)
    mapped, keep = _surviving_faces(faces, cluster, V)
    return _compact(position, new_normals, new_colors, mapped, keep, cluster, return_index)


def _simplify_scalar(verts, faces, voxel, normals=None, colors=None, contraction="quadric", return_index=False):
    """``simplify_mesh`` as a loop over the clusters in Python floats (IEEE float64, every operation rounded on its own): the definition
    read line by line.  Slow; the tests hold ``simplify_mesh`` equal to it bit for bit."""
    verts, faces, voxel, normals, colors, contraction = _arguments(verts, faces, voxel, normals, colors, contraction)
    V, F = len(verts), len(faces)
    if V == 0:
        return _empty(V, normals, colors, return_index)
    keys, _, _ = voxel_keys(verts, voxel)
    members = {}
    for i in range(V):                                           # ascending vertex index within every cluster
        members.setdefault(int(keys[i]), []).append(i)
    ordered = sorted(members)
    M = len(ordered)
    cluster = [0] * V
    for c, key in enumerate(ordered):
        for i in members[key]:
            cluster[i] = c
    incidences = [[] for _ in range(M)]
    for f in range(F):
        tri = [int(t) for t in faces[f]]
        if all(0 <= t < V for t in tri):
            for j in range(3):
                incidences[cluster[tri[j]]].append(f)            # ascending 3 f + j
    limit = float(np.float32(voxel))
    position = np.zeros((M, 3), np.float32)
    new_normals = None if normals is None else np.zeros((M, 3), np.float32)
    new_colors = None if colors is None else np.zeros((M, 3), np.uint8)
    for c, key in enumerate(ordered):
        mine = members[key]
        s = [0.0, 0.0, 0.0]
        for i in mine:
            for k in range(3):
                s[k] += float(verts[i][k])
        mean = [np.float32(s[k] / len(mine)) for k in range(3)]
        position[c] = mean
        if new_normals is not None:
            t = [0.0, 0.0, 0.0]
            for i in mine:
                for k in range(3):
                    t[k] += float(normals[i][k])
            sq = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]
            length = math.sqrt(sq) if sq >= 0.0 else math.nan
            if 0.0 < length < math.inf:
                new_normals[c] = [t[k] / length for k in range(3)]
        if new_colors is not None:
            for k in range(3):
                total = sum(int(colors[i][k]) for i in mine)
                new_colors[c][k] = int(np.rint(float(total) / float(len(mine))))
        if contraction != "quadric":
            continue
        o = [float(m) for m in mean]
        A = [[0.0] * 3 for _ in range(3)]
        b = [0.0, 0.0, 0.0]
        for f in incidences[c]:
            p = [[float(verts[int(faces[f][k])][a]) - o[a] for a in range(3)] for k in range(3)]
            e1 = [p[1][a] - p[0][a] for a in range(3)]
            e2 = [p[2][a] - p[0][a] for a in range(3)]
            n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
            d = -((n[0] * p[0][0] + n[1] * p[0][1]) + n[2] * p[0][2])
            for r, e in _UPPER:
                A[r][e] += n[r] * n[e]
            for r in range(3):
                b[r] += d * n[r]
        for r, e in _UPPER:
            A[e][r] = A[r][e]
        lam, Vc = _jacobi3(A)
        lmax = lam[0]
        if lam[1] > lmax:
            lmax = lam[1]
        if lam[2] > lmax:
            lmax = lam[2]
        x = [0.0, 0.0, 0.0]
        for i in range(3):
            if lam[i] > RANK_THRESHOLD * lmax:
                coef = -_div((Vc[0][i] * b[0] + Vc[1][i] * b[1]) + Vc[2][i] * b[2], lam[i])
                for k in range(3):
                    x[k] += coef * Vc[k][i]
        if lmax > 0.0 and all(abs(x[k]) <= limit for k in range(3)):
            position[c] = [np.float32(o[k] + x[k]) for k in range(3)]
    keep, seen, mapped = np.zeros(F, dtype=bool), set(), np.zeros((F, 3), np.int64)
    for f in range(F):
        tri = [int(t) for t in faces[f]]
        if not all(0 <= t < V for t in tri):
            continue
        a, b_, c_ = (cluster[t] for t in tri)
        mapped[f] = (a, b_, c_)
        if a == b_ or b_ == c_ or a == c_:
            continue
        rotations = {(a, b_, c_), (b_, c_, a), (c_, a, b_)}
        if seen & rotations:
            continue
        seen.add((a, b_, c_))
        keep[f] = True
    return _compact(position, new_normals, new_colors, mapped, keep, np.asarray(cluster, dtype=np.int64), return_index)


def _div(a, b):
    """a / b in float64 as IEEE has it where Python would raise: a zero divisor gives an infinity or a NaN."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def simplify_mesh_device(verts, faces, voxel, normals=None, colors=None, contraction="quadric", return_index=False):
    """``simplify_mesh`` for device tensors (``dvmvs.hip.simplify.simplify_mesh``): the same bits, on the GPU."""
    from dvmvs.hip import simplify
    return simplify.simplify_mesh(verts, faces, voxel, normals, colors, contraction, return_index)

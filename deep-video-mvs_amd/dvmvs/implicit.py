"""A surface for the point path: the implicit moving-least-squares (IMLS) signed distance of an oriented point cloud on a voxel grid, whose
zero level ``dvmvs.tsdf.marching_cubes`` turns into a mesh.  The cloud is the fused one (``dvmvs.consistency.fused_point_cloud``, cleaned by
``dvmvs.outliers``) with the normals of ``dvmvs.normals``; the mesh is what ``filter_components``, ``surface_sample``, ``render_mesh`` and
``score_against`` take.  The function is evaluated only in the band of nodes around the points; every other node holds a positive fill,
and the crossings that marching cubes finds between the band and the fill are trimmed away (``trim_mesh``).

This module is the host definition, in numpy, importable without a GPU.  ``implicit_volume_device``, ``trim_mesh_device`` and
``mesh_points_device`` are the same on the GPU (``dvmvs.hip.implicit``, csrc/implicit_surface.hip) and give the same bits.

Arithmetic contract (include/dvmvs_hip.h states it for the C entries).  ``voxel`` and ``radius`` are float32 numbers (what is given is
rounded to float32 once).  Unless said otherwise everything is float64 computed from the float32 inputs with +, -, * and / only, every
operation rounded on its own, nothing fused.

Grid: ``origin`` float32 [3], ``voxel`` > 0, ``dims = (X, Y, Z)``, z fastest as everywhere in ``dvmvs.tsdf``.  Node (i, j, k) lies at
``x_c = fl32(fl32(fl32(i_c) * voxel) + origin_c)``: both steps in float32, each rounded once.  That float32 position is the query of the
search.

Rows: ``nearest_neighbours(nodes, points, neighbours, radius, exclude_same_index=False)`` of ``dvmvs.outliers``, unchanged: the
``neighbours`` (1 .. 32) nearest points within ``radius`` (finite, > 0) under its float32 test, sorted by ``(d2, j)``.

Per node, over its row in slot order.  A slot is USED when ``0 <= j < M`` and ``normals[j] != (0, 0, 0)`` (the invalid normals of
``estimate_normals`` are zero).  ``h2 = float64(radius) * float64(radius)``.  For each used slot:
1. ``e = x - points[j]``, exact in float64
2. ``d2 = (e_x e_x + e_y e_y) + e_z e_z``
3. ``t = 1 - d2 / h2``; ``t < 0`` becomes 0 (the slot still counts as used: the float32 test of the search and this float64 one may differ
   in the last place)
4. ``w = (t t) t``
5. ``s = (n_x e_x + n_y e_y) + n_z e_z``
6. ``num += w s`` and ``den += w``, both from 0.0
The node is VALID when at least ``min_neighbours`` (>= 1) slots were used and ``den > 0``; then ``value = float32(num / den)``.  Any other
node gets ``value = float32(radius)``, a positive fill: an invalid node is never inside.  The weight has no exp, sqrt or trigonometry, so
that the device can give numpy's bits.  ``value`` grows along the normals.  Coordinates and normals must be finite."""
import numpy as np

from dvmvs.outliers import MAX_NEIGHBOURS, nearest_neighbours

MAX_NODES = 2 ** 31                  # the limit of marching cubes
DEFAULT_NEIGHBOURS = 32
DEFAULT_MIN_NEIGHBOURS = 3


def _count(name, label, value, low, high):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not low <= int(value) <= high:
        raise ValueError(f"{name}: {label} must be an integer in [{low}, {high}], got {value!r}")
    return int(value)


def _length(name, label, value):
    """``value`` as a float32 that is finite and > 0."""
    try:
        value = np.float32(value)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"{name}: {label} must be a length, got {value!r}") from None
    if value.ndim != 0 or not np.isfinite(value) or not value > 0.0:
        raise ValueError(f"{name}: {label} must be finite and > 0, got {value!r}")
    return value


def _cloud(name, points, normals):
    points = np.ascontiguousarray(points, dtype=np.float32)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"{name}: points must be float32 [M,3], got {points.shape}")
    normals = np.ascontiguousarray(normals, dtype=np.float32)
    if normals.shape != points.shape:
        raise ValueError(f"{name}: normals must be float32 {list(points.shape)}, one for every point, got {normals.shape}")
    if len(points) == 0:
        raise ValueError(f"{name}: the cloud is empty")
    return points, normals


def _grid(name, origin, voxel, dims):
    try:
        origin = np.ascontiguousarray(origin, dtype=np.float32)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: origin must be float32 [3], got {origin!r}") from None
    if origin.shape != (3,) or not np.isfinite(origin).all():
        raise ValueError(f"{name}: origin must be three finite float32 numbers, got {origin!r}")
    voxel = _length(name, "voxel", voxel)
    try:
        dims = tuple(dims)
    except TypeError:
        raise ValueError(f"{name}: dims must be three whole numbers (X, Y, Z), got {dims!r}") from None
    if len(dims) != 3:
        raise ValueError(f"{name}: dims must be three whole numbers (X, Y, Z), got {dims!r}")
    dims = tuple(_count(name, "each of dims", d, 0, MAX_NODES) for d in dims)
    if dims[0] * dims[1] * dims[2] > MAX_NODES:
        raise ValueError(f"{name}: a grid of {dims[0]}x{dims[1]}x{dims[2]} nodes is more than 2^31, the limit of marching cubes")
    return origin, voxel, dims


def _settings(name, radius, neighbours, min_neighbours):
    return (_length(name, "radius", radius), _count(name, "neighbours", neighbours, 1, MAX_NEIGHBOURS),
            _count(name, "min_neighbours", min_neighbours, 1, 2 ** 31 - 1))


def node_positions(origin, voxel, dims):
    """float32 [X*Y*Z,3]: the nodes of the grid, z fastest, ``fl32(fl32(fl32(i) * voxel) + origin)`` on every axis."""
    origin, voxel, dims = _grid("node_positions", origin, voxel, dims)
    axes = [np.arange(d).astype(np.float32) * voxel + origin[c] for c, d in enumerate(dims)]       # float32 arrays: two rounded steps
    return np.stack([a.reshape(-1) for a in np.meshgrid(*axes, indexing="ij")], axis=1).astype(np.float32)


def _implicit_values(nodes, points, normals, index, radius, min_neighbours):
    """``(value float32 [A], valid bool [A])`` of the nodes from their rows, vectorised over the nodes: elementwise float64 operations of
    numpy are the correctly rounded ones, so the bits are those of ``_implicit_value_scalar``."""
    A, M = len(nodes), len(points)
    x = nodes.astype(np.float64)
    p64, n64 = points.astype(np.float64), normals.astype(np.float64)
    has_normal = (normals != 0.0).any(axis=1)
    h2 = np.float64(radius) * np.float64(radius)
    num, den, used = np.zeros(A), np.zeros(A), np.zeros(A, dtype=np.int64)
    index = index.astype(np.int64)
    for slot in range(index.shape[1]):
        j = index[:, slot]
        inside = (j >= 0) & (j < M)
        j = np.where(inside, j, 0)
        ok = inside & has_normal[j]
        e = x - p64[j]
        n = n64[j]
        d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        t = 1.0 - d2 / h2
        t = np.where(t < 0.0, 0.0, t)
        w = (t * t) * t
        s = (n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1]) + n[:, 2] * e[:, 2]
        num = np.where(ok, num + w * s, num)
        den = np.where(ok, den + w, den)
        used += ok
    valid = (used >= min_neighbours) & (den > 0.0)
    value = np.where(valid, num / np.where(valid, den, 1.0), 0.0).astype(np.float32)
    return np.where(valid, value, np.float32(radius)).astype(np.float32), valid


def _implicit_value_scalar(node, points, normals, row, radius, min_neighbours):
    """``(value float32, valid bool)`` of ONE node (float32 [3]) from its row, in Python floats (IEEE float64, every operation rounded on its
    own): the definition read line by line.  Slow; the tests hold ``implicit_volume`` equal to it bit for bit."""
    M = len(points)
    x = [float(c) for c in node]
    h2 = float(np.float32(radius)) * float(np.float32(radius))
    num, den, used = 0.0, 0.0, 0
    for j in row:
        j = int(j)
        if not 0 <= j < M:
            continue
        n = [float(c) for c in normals[j]]
        if n[0] == 0.0 and n[1] == 0.0 and n[2] == 0.0:
            continue
        e = [x[c] - float(points[j][c]) for c in range(3)]
        d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        t = 1.0 - d2 / h2
        if t < 0.0:
            t = 0.0
        w = (t * t) * t
        s = (n[0] * e[0] + n[1] * e[1]) + n[2] * e[2]
        num += w * s
        den += w
        used += 1
    if used >= min_neighbours and den > 0.0:
        return np.float32(num / den), True
    return np.float32(radius), False


def implicit_volume(points, normals, origin, voxel, dims, radius, neighbours=DEFAULT_NEIGHBOURS, min_neighbours=DEFAULT_MIN_NEIGHBOURS):
    """``(volume float32 [X,Y,Z], valid bool [X,Y,Z])``: the module's signed distance of the cloud ``points`` float32 [M,3] with ``normals``
    float32 [M,3] at EVERY node of the grid (``origin`` float32 [3], ``voxel``, ``dims = (X, Y, Z)``), searched densely: a brute force,
    for small grids.  An invalid node holds ``float32(radius)``."""
    name = "implicit_volume"
    points, normals = _cloud(name, points, normals)
    origin, voxel, dims = _grid(name, origin, voxel, dims)
    radius, neighbours, min_neighbours = _settings(name, radius, neighbours, min_neighbours)
    if dims[0] * dims[1] * dims[2] == 0:
        return np.zeros(dims, np.float32), np.zeros(dims, bool)
    nodes = node_positions(origin, voxel, dims)
    index = nearest_neighbours(nodes, points, neighbours, radius, False)[1]
    value, valid = _implicit_values(nodes, points, normals, index, radius, min_neighbours)
    return value.reshape(dims), valid.reshape(dims)


def _grid_from_box(name, low, high, voxel, radius):
    """``grid_for`` from the cloud's box ``low``, ``high`` (float32 [3] each)."""
    voxel, radius = np.float64(_length(name, "voxel", voxel)), np.float64(_length(name, "radius", radius))
    low, high = np.asarray(low, dtype=np.float32).astype(np.float64), np.asarray(high, dtype=np.float32).astype(np.float64)
    if not (np.isfinite(low).all() and np.isfinite(high).all()):
        raise ValueError(f"{name}: the cloud's coordinates must be finite, got a box from {low} to {high}")
    lo = np.floor((low - radius) / voxel)
    hi = np.ceil((high + radius) / voxel)
    extent = hi - lo + 1.0
    if not (extent < 2.0 ** 31).all() or extent[0] * extent[1] * extent[2] > MAX_NODES:
        raise ValueError(f"{name}: the cloud needs a grid of {extent[0]:.0f}x{extent[1]:.0f}x{extent[2]:.0f} nodes at voxel {voxel:g}, more "
                         f"than 2^31, the limit of marching cubes")
    return (lo * voxel).astype(np.float32), tuple(int(d) for d in extent)


def grid_for(points, voxel, radius):
    """``(origin float32 [3], dims)`` of the grid that holds every node within ``radius`` of the cloud ``points`` float32 [M,3]: in float64
    ``lo_c = floor((min_c - radius) / voxel)``, ``hi_c = ceil((max_c + radius) / voxel)``, ``origin_c = float32(lo_c * voxel)``,
    ``dims_c = hi_c - lo_c + 1``.  ``ValueError`` for an empty cloud and for more than 2^31 nodes, the limit of marching cubes."""
    name = "grid_for"
    points = np.ascontiguousarray(points, dtype=np.float32)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"{name}: points must be float32 [M,3], got {points.shape}")
    if len(points) == 0:
        raise ValueError(f"{name}: the cloud is empty")
    return _grid_from_box(name, points.min(axis=0), points.max(axis=0), voxel, radius)


def trim_mesh(verts_index, faces, valid):
    """``(verts_index', faces', kept_vertex int64 [V'])``: the mesh of ``marching_cubes(volume, 0.0, None, (0, 0, 0), 1.0)`` (vertices in
    index space: two coordinates of a vertex are whole numbers, the third lies on a grid edge) without what the fill invented.  A vertex
    is kept when the nodes ``floor(pos)`` and ``ceil(pos)`` (componentwise; one node when the vertex sits exactly on it) are both valid
    (and inside the grid), a face when its three vertices are.  Kept vertices and faces keep their order, faces are re-indexed;
    ``kept_vertex`` holds the old indices of the kept vertices.

    Sufficient because every invented crossing lies on an edge with an invalid endpoint (invalid nodes hold the positive fill, so a sign
    change between two valid nodes is the function's own), and harmless because a node with ``value < 0`` is always valid: a crossing
    between two valid nodes is never removed."""
    name = "trim_mesh"
    verts_index = np.ascontiguousarray(verts_index, dtype=np.float32)
    faces = np.asarray(faces)
    valid = np.asarray(valid)
    if verts_index.ndim != 2 or verts_index.shape[1] != 3:
        raise ValueError(f"{name}: verts_index must be float32 [V,3], got {verts_index.shape}")
    if faces.ndim != 2 or faces.shape[1] != 3 or not np.issubdtype(faces.dtype, np.integer):
        raise ValueError(f"{name}: faces must be an integer array [F,3], got {faces.dtype} {faces.shape}")
    if valid.ndim != 3 or valid.dtype != bool:
        raise ValueError(f"{name}: valid must be bool [X,Y,Z], got {valid.dtype} {valid.shape}")
    V = len(verts_index)
    if len(faces) and (faces.min() < 0 or faces.max() >= V):
        raise ValueError(f"{name}: faces index vertices outside [0, {V})")
    keep = np.ones(V, dtype=bool)
    limit = np.array(valid.shape, dtype=np.float64)
    for corner in (np.floor(verts_index), np.ceil(verts_index)):
        inside = ((corner >= 0) & (corner < limit)).all(axis=1)
        node = np.where(inside[:, None], corner, 0).astype(np.int64)
        keep &= inside & valid[node[:, 0], node[:, 1], node[:, 2]] if valid.size else inside & False
    keep_face = keep[faces].all(axis=1) if len(faces) else np.zeros(0, dtype=bool)
    new_index = np.cumsum(keep) - 1
    return verts_index[keep], new_index[faces[keep_face]].astype(faces.dtype).reshape(-1, 3), np.flatnonzero(keep).astype(np.int64)


def implicit_volume_device(points, normals, origin, voxel, dims, radius, neighbours=DEFAULT_NEIGHBOURS,
                           min_neighbours=DEFAULT_MIN_NEIGHBOURS):
    """``implicit_volume`` for device tensors (``dvmvs.hip.implicit.implicit_volume``): the same bits, on the GPU, searched only in the
    band of nodes around the points."""
    from dvmvs.hip import implicit
    return implicit.implicit_volume(points, normals, origin, voxel, dims, radius, neighbours, min_neighbours)


def trim_mesh_device(verts_index, faces, valid):
    """``trim_mesh`` for device tensors (``dvmvs.hip.implicit.trim_mesh``): the same mesh, on the GPU."""
    from dvmvs.hip import implicit
    return implicit.trim_mesh(verts_index, faces, valid)


def mesh_points_device(cloud, normals, voxel, radius, neighbours=DEFAULT_NEIGHBOURS, min_neighbours=DEFAULT_MIN_NEIGHBOURS, bounds=None,
                       clean=None):
    """The mesh of an oriented cloud on the GPU (``dvmvs.hip.implicit.mesh_points``): ``(verts float32 [V,3], faces int32 [F,3], normals
    float32 [V,3], colors uint8 [V,3] or None)``, the tuple of ``dvmvs.tsdf.marching_cubes``."""
    from dvmvs.hip import implicit
    return implicit.mesh_points(cloud, normals, voxel, radius, neighbours, min_neighbours, bounds, clean)

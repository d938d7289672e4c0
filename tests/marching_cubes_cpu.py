"""CPU restatement of the marching-cubes contract of csrc/marching_cubes.hip, vectorised with numpy (no per-cube Python loop).

The case tables are read from csrc/marching_cubes_tables.h, their only copy.  Same float32 arithmetic, statement by statement, as
the kernel (which compiles it with contraction off), so the HIP output is compared array for array:
  - inside: value < level; a vertex on every grid edge with exactly one inside endpoint;
  - vertex order: (linear index of the owning voxel, axis x < y < z) -- each voxel owns its +x, +y, +z edges;
  - t = (level - v_a) / (v_b - v_a), index-space p = float(i) + t, world = p * voxel_size + origin;
  - normal = g_a + t * (g_b - g_a) with np.gradient's g, / sqrt(nx*nx + ny*ny + nz*nz); a zero length gives the zero vector;
  - colour = the colour voxel at np.rint(p), decoded like the reference's get_mesh;
  - faces: cubes by the linear index of their lowest corner, then table order.
"""
import os
import re

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
TABLES_H = os.path.join(ROOT, "deep-video-mvs_amd", "csrc", "marching_cubes_tables.h")

_TABLES = None


def tables():
    """{'edge_corners' [12,2], 'edge_owner' [12,4], 'edge_table' [256], 'tri_count' [256], 'tri_table' [256,W]} from the header."""
    global _TABLES
    if _TABLES is None:
        text = re.sub(r"//[^\n]*", "", open(TABLES_H).read())
        out = {}
        for key, name, shape in (("edge_corners", "kMcEdgeCorners", (12, 2)), ("edge_owner", "kMcEdgeOwner", (12, 4)),
                                 ("edge_table", "kMcEdgeTable", (256,)), ("tri_count", "kMcTriCount", (256,)),
                                 ("tri_table", "kMcTriTable", None)):
            m = re.search(name + r"((?:\[\d+\])+)\s*=\s*\{(.*?)\};", text, flags=re.S)
            dims = tuple(int(d) for d in re.findall(r"\d+", m.group(1)))
            vals = [int(v, 0) for v in re.findall(r"-?(?:0x[0-9a-fA-F]+|\d+)", m.group(2))]
            out[key] = np.array(vals, dtype=np.int64).reshape(dims)
            assert shape is None or dims == shape
        _TABLES = out
    return _TABLES


def _decode_colors(rgb_vals):
    """The reference's get_mesh colour decoding (float32 arithmetic) -> uint8 [N,3] RGB."""
    b = np.floor(rgb_vals / np.float32(65536))
    g = np.floor((rgb_vals - b * np.float32(65536)) / np.float32(256))
    r = rgb_vals - b * np.float32(65536) - g * np.float32(256)
    return np.floor(np.asarray([r, g, b])).T.astype(np.uint8)


def marching_cubes(volume, level=0.0, color=None, origin=(0.0, 0.0, 0.0), voxel_size=1.0):
    """(verts float32 [V,3], faces int32 [F,3], normals float32 [V,3], colors uint8 [V,3] or None) of a float32 [X,Y,Z] volume."""
    vol = np.ascontiguousarray(volume, dtype=np.float32)
    level = np.float32(level)
    vs = np.float32(voxel_size)
    org = np.asarray(origin, dtype=np.float32).reshape(3)
    X, Y, Z = vol.shape
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32),
             None if color is None else np.zeros((0, 3), np.uint8))
    if min(X, Y, Z) < 2:
        return empty
    tab = tables()
    inside = vol < level
    owned = np.zeros((X, Y, Z, 3), dtype=bool)
    owned[:-1, :, :, 0] = inside[:-1] != inside[1:]
    owned[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    owned[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    flat = np.flatnonzero(owned.reshape(-1))
    V = len(flat)
    if V == 0:
        return empty
    vid = np.full(X * Y * Z * 3, -1, dtype=np.int64)
    vid[flat] = np.arange(V)
    lin, axis = flat // 3, flat % 3
    a = np.stack(np.unravel_index(lin, (X, Y, Z)), axis=1)          # [V,3] owner voxel
    b = a.copy()
    b[np.arange(V), axis] += 1
    va, vb = vol[a[:, 0], a[:, 1], a[:, 2]], vol[b[:, 0], b[:, 1], b[:, 2]]
    t = (level - va) / (vb - va)
    p = a.astype(np.float32)
    p[np.arange(V), axis] = p[np.arange(V), axis] + t
    verts = p * vs + org
    grads = np.gradient(vol)
    ga = np.stack([g[a[:, 0], a[:, 1], a[:, 2]] for g in grads], axis=1)
    gb = np.stack([g[b[:, 0], b[:, 1], b[:, 2]] for g in grads], axis=1)
    n = ga + t[:, None] * (gb - ga)
    length = np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        normals = np.where(length[:, None] == 0, np.float32(0), n / length[:, None]).astype(np.float32)
    colors = None
    if color is not None:
        q = np.rint(p).astype(np.int64)
        colors = _decode_colors(np.asarray(color, dtype=np.float32)[q[:, 0], q[:, 1], q[:, 2]])

    # cubes: case index from the 8 corners (bit c <=> corner c inside), kept in the order of their lowest corner
    cin = inside.astype(np.int64)
    corners = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
    case = np.zeros((X - 1, Y - 1, Z - 1), dtype=np.int64)
    for c, (di, dj, dk) in enumerate(corners):
        case |= cin[di:X - 1 + di, dj:Y - 1 + dj, dk:Z - 1 + dk] << c
    ntri = tab["tri_count"][case]
    cubes = np.flatnonzero(ntri.reshape(-1))                           # cube order = order of the lowest corner's linear index
    if len(cubes) == 0:
        return verts, np.zeros((0, 3), np.int32), normals, colors
    ci = np.stack(np.unravel_index(cubes, (X - 1, Y - 1, Z - 1)), axis=1)
    cc = case.reshape(-1)[cubes]
    width = tab["tri_table"].shape[1]
    rows = tab["tri_table"][cc][:, :width - 1].reshape(len(cubes), -1, 3)
    valid = np.arange(rows.shape[1])[None, :] < ntri.reshape(-1)[cubes][:, None]
    edges = rows[valid]                                                # [F,3], cube-major, table order
    cube_of = np.repeat(np.arange(len(cubes)), valid.sum(1))
    own = tab["edge_owner"][edges]                                     # [F,3,4]
    o = ci[cube_of][:, None, :] + own[..., :3]
    key = ((o[..., 0] * Y + o[..., 1]) * Z + o[..., 2]) * 3 + own[..., 3]
    faces = vid[key]
    assert (faces >= 0).all()
    return verts, faces.astype(np.int32), normals, colors

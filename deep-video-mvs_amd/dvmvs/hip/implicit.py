"""The implicit signed distance of an oriented point cloud and its mesh on the device (csrc/implicit_surface.hip; definition in
include/dvmvs_hip.h, host form in dvmvs/implicit.py): plain functions over the C ABI and the ops package's launch plumbing, on top of the
k-NN search of ``dvmvs.hip.neighbours``, ``dvmvs.tsdf.marching_cubes`` and the nearest-point query.  Inference-time geometry only: nothing
here is registered under ``torch.ops.dvmvs`` and nothing needs autograd."""
from typing import Optional

import numpy as np
import torch
from torch import Tensor

from dvmvs import implicit as _host
from dvmvs.hip import neighbours as _neighbours
from dvmvs.hip.ops._common import check_tensors, launch, ptr
from dvmvs.hip.ops.reconstruction import nearest_build, nearest_query
from dvmvs.hip.volume import marching_cubes
from dvmvs.implicit import DEFAULT_MIN_NEIGHBOURS, DEFAULT_NEIGHBOURS

MAX_POINTS = 1 << 28


def _cloud(name, points, normals):
    check_tensors(name, points, label="points", shape=(None, 3))
    check_tensors(name, normals, label="normals", shape=(int(points.shape[0]), 3), device=points.device)
    M = int(points.shape[0])
    if M < 1:
        raise ValueError(f"dvmvs::{name}: the cloud is empty")
    if M > MAX_POINTS:
        raise ValueError(f"dvmvs::{name}: {M} points are outside what the kernels take (2^28 at most)")
    return points.contiguous(), normals.contiguous(), M


def _checked(name, call, *args):
    """The host module's argument check with this module's prefix."""
    try:
        return call(name, *args)
    except ValueError as e:
        raise ValueError(f"dvmvs::{e}") from None


def band(points: Tensor, origin, voxel: float, dims, radius: float) -> Tensor:
    """uint8 [X,Y,Z]: 1 at every node of the grid that can have a point of ``points`` float32 [M,3] within ``radius`` under the float32 test
    of the search, and possibly at more (the cube around every point; csrc/implicit_surface.hip derives the reach).  One fill and one
    launch on the current stream, nothing read by the host."""
    name = "implicit_band"
    check_tensors(name, points, label="points", shape=(None, 3))
    origin, voxel, dims = _checked(name, _host._grid, origin, voxel, dims)
    radius = _checked(name, _host._length, "radius", radius)
    mask = torch.zeros(dims, dtype=torch.uint8, device=points.device)
    if points.shape[0] > 0 and mask.numel() > 0:
        points = points.contiguous()
        launch("dvmvs_implicit_band_fwd", points.device, ptr(points), int(points.shape[0]), float(origin[0]), float(origin[1]),
               float(origin[2]), float(voxel), dims[0], dims[1], dims[2], float(radius), ptr(mask))
    return mask


def node_positions(linear: Tensor, origin, voxel: float, dims) -> Tensor:
    """float32 [A,3]: the positions of the nodes with the linear indices ``linear`` int64 [A] (``(i * Y + j) * Z + k``, inside the grid),
    ``fl32(fl32(fl32(i) * voxel) + origin)`` on every axis.  One launch, nothing read by the host."""
    name = "implicit_nodes"
    check_tensors(name, linear, dtype=torch.int64, label="linear", shape=(None,))
    origin, voxel, dims = _checked(name, _host._grid, origin, voxel, dims)
    linear = linear.contiguous()
    nodes = torch.empty((int(linear.shape[0]), 3), dtype=torch.float32, device=linear.device)
    if linear.shape[0] > 0:
        launch("dvmvs_implicit_nodes_fwd", linear.device, ptr(linear), int(linear.shape[0]), float(origin[0]), float(origin[1]),
               float(origin[2]), float(voxel), dims[0], dims[1], dims[2], ptr(nodes))
    return nodes


def implicit_volume(points: Tensor, normals: Tensor, origin, voxel: float, dims, radius: float, neighbours: int = DEFAULT_NEIGHBOURS,
                    min_neighbours: int = DEFAULT_MIN_NEIGHBOURS, grid: Optional[Tensor] = None, nodes_per_chunk: int = 1 << 20):
    """``dvmvs.implicit.implicit_volume`` on the device, bit for bit: ``(volume float32 [X,Y,Z], valid bool [X,Y,Z])`` of the cloud
    ``points`` float32 [M,3] with ``normals`` float32 [M,3] on the grid (``origin`` three numbers, ``voxel``, ``dims = (X, Y, Z)``).  The
    band kernel marks the candidate nodes, ``torch.nonzero`` lists them (ONE host read), and per chunk of at most ``nodes_per_chunk``
    of them: the node positions, ``neighbours.knn(nodes, points, neighbours, radius, False, grid)`` and the values kernel, which scatters
    into the volume pre-filled with ``float32(radius)``.  A node outside the band has no candidate and keeps the fill, as in the dense
    host form.  ``grid``: the ``ops.nearest_build`` workspace of ``points`` when the caller has it; it is built once otherwise.  The
    rows of a chunk take ``nodes_per_chunk * neighbours * 8`` bytes; the chunking changes no bit of the result."""
    name = "implicit_volume"
    points, normals, M = _cloud(name, points, normals)
    origin, voxel, dims = _checked(name, _host._grid, origin, voxel, dims)
    radius, neighbours, min_neighbours = _checked(name, _host._settings, radius, neighbours, min_neighbours)
    if isinstance(nodes_per_chunk, bool) or not isinstance(nodes_per_chunk, int) or not 1 <= nodes_per_chunk <= MAX_POINTS:
        raise ValueError(f"dvmvs::{name}: nodes_per_chunk must be an integer in [1, 2^28], got {nodes_per_chunk!r}")
    device = points.device
    volume = torch.full(dims, float(radius), dtype=torch.float32, device=device)
    valid = torch.zeros(dims, dtype=torch.uint8, device=device)
    total = volume.numel()
    if total == 0:
        return volume, valid.view(torch.bool)
    mask = band(points, origin, voxel, dims, radius)
    linear = torch.nonzero(mask.reshape(-1)).reshape(-1)                  # the one host read: how many candidates there are
    del mask
    if linear.numel() > 0 and grid is None:
        grid = nearest_build(points)
    for begin in range(0, int(linear.numel()), nodes_per_chunk):
        chunk = linear[begin:begin + nodes_per_chunk]
        nodes = node_positions(chunk, origin, voxel, dims)
        index = _neighbours.knn(nodes, points, neighbours, float(radius), False, grid)[1]
        launch("dvmvs_implicit_values_fwd", device, ptr(nodes), int(chunk.numel()), ptr(points), ptr(normals), M, ptr(index), neighbours,
               float(radius), min_neighbours, ptr(chunk), total, ptr(volume), ptr(valid))
    return volume, valid.view(torch.bool)


def trim_flags(verts_index: Tensor, faces: Tensor, valid: Tensor):
    """``(keep_vertex bool [V], keep_face bool [F])`` by the rule of ``dvmvs.implicit.trim_mesh``: a vertex (float32 [V,3], index space) is
    kept when the nodes ``floor(pos)`` and ``ceil(pos)`` are both valid (``valid`` bool [X,Y,Z]), a face (int32 [F,3]) when its three
    vertices are.  Two launches, nothing read by the host."""
    name = "implicit_trim"
    check_tensors(name, verts_index, label="verts_index", shape=(None, 3))
    device = verts_index.device
    check_tensors(name, faces, dtype=torch.int32, label="faces", shape=(None, 3), device=device)
    check_tensors(name, valid, dtype=(torch.bool, torch.uint8), label="valid", shape=(None, None, None), device=device)
    V, F = int(verts_index.shape[0]), int(faces.shape[0])
    keep_vertex = torch.zeros(V, dtype=torch.uint8, device=device)
    keep_face = torch.zeros(F, dtype=torch.uint8, device=device)
    if (V > 0 or F > 0) and valid.numel() > 0:
        verts_index, faces, valid = verts_index.contiguous(), faces.contiguous(), valid.contiguous()
        launch("dvmvs_implicit_trim_fwd", device, ptr(verts_index), V, ptr(faces), F, ptr(valid), int(valid.shape[0]), int(valid.shape[1]),
               int(valid.shape[2]), ptr(keep_vertex), ptr(keep_face))
    return keep_vertex.view(torch.bool), keep_face.view(torch.bool)


def trim_mesh(verts_index: Tensor, faces: Tensor, valid: Tensor):
    """``dvmvs.implicit.trim_mesh`` on the device: ``(verts_index', faces' int32, kept_vertex int64 [V'])``.  The flags are the trim
    kernel's; the compaction and the re-indexing are ``cumsum`` and boolean indexing (which reads the sizes: a synchronisation)."""
    keep_vertex, keep_face = trim_flags(verts_index, faces, valid)
    new_index = (torch.cumsum(keep_vertex, dim=0) - 1).to(torch.int32)
    kept_faces = faces[keep_face]
    return (verts_index[keep_vertex], new_index[kept_faces.long()].reshape(-1, 3) if kept_faces.numel() else kept_faces,
            torch.nonzero(keep_vertex).reshape(-1))


def mesh_points(cloud: Tensor, normals: Tensor, voxel: float, radius: float, neighbours: int = DEFAULT_NEIGHBOURS,
                min_neighbours: int = DEFAULT_MIN_NEIGHBOURS, bounds=None, clean=None):
    """The mesh of an oriented cloud: ``cloud`` float32 [N,3] or [N,6] (xyz, then rgb in 0..255 as ``fused_point_cloud`` gives) with
    ``normals`` float32 [N,3] (zero where a point has none, as ``estimate_normals`` leaves them) -> ``(verts float32 [V,3], faces int32
    [F,3], normals float32 [V,3], colors uint8 [V,3] or None)``, the tuple of ``dvmvs.tsdf.marching_cubes``, as device tensors.

    1. The grid: ``dvmvs.implicit.grid_for`` of the cloud's box (one host read), or ``bounds = (origin, dims)``; points outside a
       given grid shape only what lies inside it.
    2. ``implicit_volume`` (one host read, the number of candidate nodes).
    3. ``dvmvs.tsdf.marching_cubes(volume, 0.0, None, (0, 0, 0), 1.0)`` in index space (its own host read of the counts).
    4. The trim kernel and the compaction (one host read, the sizes): what marching cubes found between the band and the fill goes.
    5. World positions ``fl32(fl32(pos_c * voxel) + origin_c)``.
    6. The normal and the colour of a vertex are those of the nearest cloud point (``ops.nearest_query``).  The gradient normals of
       marching cubes are not used: near the band's edge they read fill values.
    7. With ``clean``, a ``dvmvs.components.ComponentFilter``: ``filter_components_device``, as for the TSDF meshes.
    ``value`` grows along the normals, toward the cameras, so the faces are counter-clockwise seen from the camera side, as for the
    TSDF.  An empty band (a radius below the distance of every node to the cloud, or no valid normal) gives V = F = 0.

    ``radius`` and ``neighbours`` go together.  The weights reach zero at ``radius``; while fewer than ``neighbours`` points lie within
    it the cap is inactive and the function is continuous.  Where more lie within, the ``neighbours`` nearest are taken (32 at most) and
    the function has small steps where that set changes.  Advice: a ``radius`` of 2 to 3 voxels on a cloud of about one point a voxel; a
    much denser cloud is better down-sampled first (``voxel_downsample``) than cut off by the cap."""
    name = "mesh_points"
    check_tensors(name, cloud, label="cloud", shape=(None, None))
    if cloud.shape[1] not in (3, 6):
        raise ValueError(f"dvmvs::{name}: cloud must be float32 [N,3] or [N,6] (xyz, rgb), got {tuple(cloud.shape)}")
    points, normals, M = _cloud(name, cloud[:, :3], normals)
    voxel = _checked(name, _host._length, "voxel", voxel)
    radius, neighbours, min_neighbours = _checked(name, _host._settings, radius, neighbours, min_neighbours)
    device = points.device
    if bounds is None:
        box = torch.stack([points.min(dim=0).values, points.max(dim=0).values]).cpu().numpy()     # a host read
        origin, dims = _checked(name, _host._grid_from_box, box[0], box[1], voxel, radius)
    else:
        origin, _, dims = _checked(name, _host._grid, bounds[0], voxel, bounds[1])
    grid = nearest_build(points)
    volume, valid = implicit_volume(points, normals, origin, voxel, dims, radius, neighbours, min_neighbours, grid)
    verts_index, faces, _, _ = marching_cubes(volume, 0.0, None, (0.0, 0.0, 0.0), 1.0)
    verts_index, faces, _ = trim_mesh(verts_index, faces, valid)
    verts = verts_index * torch.tensor(float(voxel), dtype=torch.float32, device=device)          # two rounded float32 steps
    verts = verts + torch.as_tensor(np.asarray(origin, dtype=np.float32), device=device)
    if verts.shape[0] > 0:
        nearest = nearest_query(verts, points, grid, return_index=True)[1].long()
        vertex_normals = normals[nearest]
        colors = cloud[:, 3:6][nearest].to(torch.uint8) if cloud.shape[1] == 6 else None
    else:
        vertex_normals = torch.empty((0, 3), dtype=torch.float32, device=device)
        colors = torch.empty((0, 3), dtype=torch.uint8, device=device) if cloud.shape[1] == 6 else None
    mesh = (verts, faces, vertex_normals, colors)
    if clean is not None and faces.shape[0] > 0:
        from dvmvs.components import filter_components_device
        mesh = filter_components_device(verts, faces, clean, vertex_normals, colors)
    return mesh

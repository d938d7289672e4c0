"""Simplifying a triangle mesh by vertex clustering with quadric error representatives on the device (csrc/mesh_simplify.hip; definition in
include/dvmvs_hip.h, host form in dvmvs/simplify.py): plain functions over the C ABI and the ops package's workspace and launch plumbing.
Inference-time geometry only: nothing here is registered under ``torch.ops.dvmvs`` and nothing needs autograd."""
from typing import Optional

import numpy as np
import torch
from torch import Tensor

from dvmvs.hip import _capi
from dvmvs.hip.ops import _workspace
from dvmvs.hip.ops._common import check_tensors, launch, opt_ptr, ptr
from dvmvs.simplify import SimplifySettings, _settings

STATUS_OK, STATUS_CELLS = range(2)


def _empty(dev, V, normals, colors, return_index):
    out = (torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0, 3), dtype=torch.int32, device=dev),
           None if normals is None else torch.empty((0, 3), dtype=torch.float32, device=dev),
           None if colors is None else torch.empty((0, 3), dtype=torch.uint8, device=dev))
    if not return_index:
        return out
    return out + ((torch.full((V,), -1, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev)),)


def simplify_mesh(verts: Tensor, faces: Tensor, voxel, normals: Optional[Tensor] = None, colors: Optional[Tensor] = None,
                  contraction: str = "quadric", return_index: bool = False):
    """``dvmvs.simplify.simplify_mesh`` on the device, bit for bit: ``verts`` float32 [V,3], ``faces`` int32 [F,3], ``normals`` float32 [V,3]
    and ``colors`` uint8 [V,3] (or None) on one GPU; ``voxel`` the cell edge in metres, or a ``SimplifySettings`` that brings the
    contraction too.  Returns device tensors ``(verts', faces', normals' or None, colors' or None)`` and, with ``return_index``, a fifth
    entry ``(vertex_cluster int32 [V], face_index int32 [F'])``.  The voxel keys of the vertices, the clusters, the quadrics and their
    solution, the duplicate faces and the scans are enqueued on the current stream with four stable ``torch.sort``s between them (the keys,
    the incidences by cluster, the two keys of the faces' canonical triples), then ONE host read (a synchronisation): V', F' and the
    status, to size the outputs; then the compaction launches.  Raises ``ValueError`` where the host definition does: a voxel that is not
    positive and finite, an unknown contraction, a coordinate that is not finite or a cell index of 2^21 or more."""
    name = "simplify_mesh"
    if isinstance(voxel, SimplifySettings):
        voxel, contraction = voxel
    voxel, contraction = _settings(voxel, contraction)
    inv = float(np.float32(1.0 / voxel))
    if not 0.0 < inv < float("inf"):
        raise ValueError(f"dvmvs::{name}: 1 / voxel is not a positive float32 for voxel {voxel}")
    limit = float(np.float32(voxel))
    if not 0.0 < limit < float("inf"):
        raise ValueError(f"dvmvs::{name}: voxel {voxel} is not a positive float32")
    check_tensors(name, verts, label="verts", shape=(None, 3))
    dev = verts.device
    check_tensors(name, faces, dtype=torch.int32, label="faces", shape=(None, 3), device=dev)
    V, F = int(verts.shape[0]), int(faces.shape[0])
    if normals is not None:
        check_tensors(name, normals, label="normals", shape=(V, 3), device=dev)
        normals = normals.contiguous()
    if colors is not None:
        check_tensors(name, colors, dtype=torch.uint8, label="colors", shape=(V, 3), device=dev)
        colors = colors.contiguous()
    verts, faces = verts.contiguous(), faces.contiguous()
    lib = _capi.lib()
    nbytes = lib.dvmvs_mesh_simplify_workspace_bytes(V, F)
    voxel_bytes = lib.dvmvs_voxel_downsample_workspace_bytes(V) if V else 1
    if nbytes == 0 or voxel_bytes == 0:
        raise ValueError(f"dvmvs::{name}: {V} vertices and {F} faces are outside what the kernels take (2^28 at most)")
    if V == 0:
        return _empty(dev, V, normals, colors, return_index)
    voxel_workspace = _workspace.grown("voxel_downsample", dev, voxel_bytes, torch.uint8)
    workspace = _workspace.grown("mesh_simplify", dev, nbytes, torch.int64)
    nbytes = workspace.numel() * 8

    # the clusters: dvmvs.hip.ops.voxel_downsample's keys, sort and runs, of the vertices
    keys = torch.empty(V, dtype=torch.int64, device=dev)
    launch("dvmvs_voxel_keys", dev, ptr(verts), V, inv, ptr(voxel_workspace), voxel_workspace.numel(), ptr(keys))
    sorted_keys, sorted_index = torch.sort(keys, stable=True)
    voxel_counts = torch.empty(2, dtype=torch.int64, device=dev)
    launch("dvmvs_voxel_downsample_count", dev, ptr(verts), V, ptr(sorted_keys), ptr(sorted_index), ptr(voxel_workspace), voxel_workspace.numel(),
           ptr(voxel_counts))

    incidence_keys = torch.empty(3 * F, dtype=torch.int32, device=dev)
    third = torch.empty(F, dtype=torch.int32, device=dev)
    pair = torch.empty(F, dtype=torch.int64, device=dev)
    launch("dvmvs_mesh_simplify_keys", dev, opt_ptr(faces if F else None), V, F, ptr(sorted_index), ptr(voxel_workspace), ptr(voxel_counts),
           ptr(workspace), nbytes, opt_ptr(incidence_keys if F else None), opt_ptr(third if F else None), opt_ptr(pair if F else None))
    incidence_sorted = incidence_order = third_order = pair_sorted = pair_order = None
    if F:
        if contraction == "quadric":
            incidence_sorted, incidence_order = torch.sort(incidence_keys, stable=True)
        else:                                         # the average needs no incidence: nothing reads the sorted keys
            incidence_sorted, incidence_order = incidence_keys, torch.empty(3 * F, dtype=torch.int64, device=dev)
        _, third_order = torch.sort(third, stable=True)
        pair_in_order = torch.empty(F, dtype=torch.int64, device=dev)
        launch("dvmvs_mesh_simplify_pair_keys", dev, ptr(pair), ptr(third_order), F, ptr(pair_in_order))
        pair_sorted, pair_order = torch.sort(pair_in_order, stable=True)
    counts = torch.empty(3, dtype=torch.int64, device=dev)
    launch("dvmvs_mesh_simplify_count", dev, ptr(verts), opt_ptr(normals), opt_ptr(colors), V, opt_ptr(faces if F else None), F, limit,
           int(contraction == "average"), ptr(sorted_index), ptr(voxel_workspace), ptr(voxel_counts), opt_ptr(incidence_sorted),
           opt_ptr(incidence_order), opt_ptr(third if F else None), opt_ptr(third_order), opt_ptr(pair_sorted), opt_ptr(pair_order),
           ptr(workspace), nbytes, ptr(counts))
    V_out, F_out, status = (int(c) for c in counts.cpu())             # the one host read
    if status != STATUS_OK:
        raise ValueError(f"dvmvs::{name}: the vertices span 2^21 voxels or more on an axis (or hold a coordinate that is not finite)")
    verts_out = torch.empty((V_out, 3), dtype=torch.float32, device=dev)
    faces_out = torch.empty((F_out, 3), dtype=torch.int32, device=dev)
    normals_out = None if normals is None else torch.empty((V_out, 3), dtype=torch.float32, device=dev)
    colors_out = None if colors is None else torch.empty((V_out, 3), dtype=torch.uint8, device=dev)
    vertex_cluster = torch.empty(V, dtype=torch.int32, device=dev) if return_index else None
    face_index = torch.empty(F_out, dtype=torch.int32, device=dev) if return_index else None
    if V_out > 0 or return_index:
        launch("dvmvs_mesh_simplify_emit", dev, V, F, ptr(workspace), nbytes, V_out, F_out, opt_ptr(verts_out if V_out else None),
               opt_ptr(faces_out if F_out else None), opt_ptr(normals_out if V_out else None), opt_ptr(colors_out if V_out else None),
               opt_ptr(vertex_cluster), opt_ptr(face_index if F_out else None))
    out = (verts_out, faces_out, normals_out, colors_out)
    return out + ((vertex_cluster, face_index),) if return_index else out

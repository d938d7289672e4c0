"""Connected components of a triangle mesh and their removal by size on the device (csrc/mesh_components.hip; definition in
include/dvmvs_hip.h, host form in dvmvs/components.py): plain functions over the C ABI and the ops package's workspace and launch plumbing.
Inference-time geometry only: nothing here is registered under ``torch.ops.dvmvs`` and nothing needs autograd."""
from typing import Optional

import torch
from torch import Tensor

from dvmvs.components import ComponentFilter, filter_settings
from dvmvs.hip import _capi
from dvmvs.hip.ops import _workspace
from dvmvs.hip.ops._common import check_tensors, launch, opt_ptr, ptr

STATUS_OK, STATUS_AREA, STATUS_GAVE_UP = range(3)
MAX_ELEMENTS = 1 << 28


def _workspace_for(name, dev, V, F):
    nbytes = _capi.lib().dvmvs_mesh_components_workspace_bytes(V, F)
    if nbytes == 0:
        raise ValueError(f"dvmvs::{name}: {V} vertices and {F} faces are outside what the kernels take (2^28 at most)")
    return _workspace.grown("mesh_components", dev, nbytes, torch.int64)


def _label(name, faces, V, verts, workspace):
    """The labelling launches: ``(labels, face_labels, face_count, area or None, result)``, all on the device."""
    dev = faces.device
    F = int(faces.shape[0])
    labels = torch.empty(V, dtype=torch.int32, device=dev)
    face_labels = torch.empty(F, dtype=torch.int32, device=dev)
    face_count = torch.empty(V, dtype=torch.int32, device=dev)
    area = None if verts is None else torch.empty(V, dtype=torch.int64, device=dev)
    result = torch.empty(2, dtype=torch.int64, device=dev)
    launch("dvmvs_mesh_components_fwd", dev, opt_ptr(verts if V else None), V, opt_ptr(faces if F else None), F, ptr(workspace),
           workspace.numel() * 8, opt_ptr(labels if V else None), opt_ptr(face_labels if F else None), opt_ptr(face_count if V else None),
           opt_ptr(area if V else None), ptr(result))
    return labels, face_labels, face_count, area, result


def _mesh(name, faces, n_verts, verts):
    check_tensors(name, faces, dtype=torch.int32, label="faces", shape=(None, 3))
    dev = faces.device
    V = int(n_verts)
    if verts is not None:
        check_tensors(name, verts, label="verts", shape=(V, 3), device=dev)
        verts = verts.contiguous()
    if V < 0:
        raise ValueError(f"dvmvs::{name}: n_verts must not be negative, got {V}")
    return faces.contiguous(), V, verts


def mesh_components(faces: Tensor, n_verts: int, verts: Optional[Tensor] = None):
    """``dvmvs.components.mesh_components`` on the device, bit for bit: ``faces`` int32 [F,3] on the GPU, ``verts`` float32 [n_verts,3] or
    None.  Returns a dict of DEVICE tensors: ``labels`` int32 [V], ``face_labels`` int32 [F], ``face_count`` int32 [V], with ``verts``
    ``area`` int64 [V], ``n_components`` (an int64 scalar) and ``status`` (an int64 scalar: 0; 1 where the host definition raises
    ``ValueError``, a face whose area is not finite or a total of 2^63 units, and the areas are then not to be used; 2 when the labelling
    gave up, which ``filter_components`` turns into a ``RuntimeError``).  Six launches on the current stream and NO host read, so an error
    is that ``status`` and not an exception."""
    name = "mesh_components"
    faces, V, verts = _mesh(name, faces, n_verts, verts)
    workspace = _workspace_for(name, faces.device, V, int(faces.shape[0]))
    labels, face_labels, face_count, area, result = _label(name, faces, V, verts, workspace)
    out = {"labels": labels, "face_labels": face_labels, "face_count": face_count, "n_components": result[0], "status": result[1]}
    if area is not None:
        out["area"] = area
    return out


def filter_components(verts: Tensor, faces: Tensor, filter: ComponentFilter, normals: Optional[Tensor] = None, colors: Optional[Tensor] = None,
                      return_index: bool = False):
    """``dvmvs.components.filter_components`` on the device, bit for bit: ``verts`` float32 [V,3], ``faces`` int32 [F,3], ``normals`` float32
    [V,3] and ``colors`` uint8 [V,3] (or None) on one GPU; returns device tensors ``(verts', faces', normals' or None, colors' or None)``
    and, with ``return_index``, a fifth entry ``(vertex_index int32 [V'], face_index int32 [F'])``.  The labelling, the decision and the
    scans are enqueued on the current stream, then ONE host read (a synchronisation): V', F' and the status, to size the outputs; then
    the two compaction launches.  Raises ``ValueError`` where the host definition does (a face whose area is not finite, a total area of
    2^63 units, bad filter settings) and ``RuntimeError`` when the labelling gave up (status 2: a union met its retry limit)."""
    name = "filter_components"
    min_area, min_faces, keep_largest = filter_settings(filter)
    check_tensors(name, verts, label="verts", shape=(None, 3))
    dev = verts.device
    check_tensors(name, faces, dtype=torch.int32, label="faces", shape=(None, 3), device=dev)
    faces, V, verts = _mesh(name, faces, verts.shape[0], verts)
    if normals is not None:
        check_tensors(name, normals, label="normals", shape=(V, 3), device=dev)
        normals = normals.contiguous()
    if colors is not None:
        check_tensors(name, colors, dtype=torch.uint8, label="colors", shape=(V, 3), device=dev)
        colors = colors.contiguous()
    F = int(faces.shape[0])
    workspace = _workspace_for(name, dev, V, F)
    nbytes = workspace.numel() * 8
    labels, face_labels, face_count, area, result = _label(name, faces, V, verts, workspace)
    counts = torch.empty(3, dtype=torch.int64, device=dev)
    launch("dvmvs_mesh_filter_count", dev, opt_ptr(labels if V else None), opt_ptr(face_labels if F else None), opt_ptr(face_count if V else None),
           opt_ptr(area if V else None), ptr(result), V, F, min_area, min_faces, int(keep_largest), ptr(workspace), nbytes, ptr(counts))
    V_out, F_out, status = (int(c) for c in counts.cpu())             # the one host read
    if status == STATUS_AREA:
        raise ValueError(f"dvmvs::{name}: a face's area is not finite or the mesh is larger than 2^31 square metres")
    if status != STATUS_OK:
        raise RuntimeError(f"dvmvs::{name}: the labelling gave up (status {status}): a union met its retry limit")
    verts_out = torch.empty((V_out, 3), dtype=torch.float32, device=dev)
    faces_out = torch.empty((F_out, 3), dtype=torch.int32, device=dev)
    normals_out = None if normals is None else torch.empty((V_out, 3), dtype=torch.float32, device=dev)
    colors_out = None if colors is None else torch.empty((V_out, 3), dtype=torch.uint8, device=dev)
    vertex_index = torch.empty(V_out, dtype=torch.int32, device=dev) if return_index else None
    face_index = torch.empty(F_out, dtype=torch.int32, device=dev) if return_index else None
    if V_out > 0 or F_out > 0:
        launch("dvmvs_mesh_filter_emit", dev, ptr(verts), ptr(faces), opt_ptr(normals), opt_ptr(colors), ptr(labels), ptr(face_labels),
               ptr(face_count), ptr(area), V, F, min_area, min_faces, int(keep_largest), ptr(workspace), nbytes, V_out, F_out, ptr(verts_out),
               ptr(faces_out), opt_ptr(normals_out), opt_ptr(colors_out), opt_ptr(vertex_index), opt_ptr(face_index))
    out = (verts_out, faces_out, normals_out, colors_out)
    return out + ((vertex_index, face_index),) if return_index else out

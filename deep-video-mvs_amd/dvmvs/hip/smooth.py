"""Smoothing a triangle mesh by the Laplacian and Taubin filters, and vertex normals from the faces, on the device (csrc/mesh_smooth.hip;
definition in include/dvmvs_hip.h, host form in dvmvs/smooth.py): plain functions over the C ABI and the ops package's workspace and launch
plumbing.  Inference-time geometry only: nothing here is registered under ``torch.ops.dvmvs`` and nothing needs autograd."""
from typing import Optional

import torch
from torch import Tensor

from dvmvs.hip import _capi
from dvmvs.hip.ops import _workspace
from dvmvs.hip.ops._common import check_tensors, launch, opt_ptr, ptr
from dvmvs.smooth import MAX_ELEMENTS, SmoothSettings, _settings


def _mesh(name, verts, faces):
    """``(verts, faces, V, F, device)`` of a checked mesh, contiguous."""
    check_tensors(name, verts, label="verts", shape=(None, 3))
    dev = verts.device
    check_tensors(name, faces, dtype=torch.int32, label="faces", shape=(None, 3), device=dev)
    return verts.contiguous(), faces.contiguous(), int(verts.shape[0]), int(faces.shape[0]), dev


def _workspace_of(name, dev, V, F):
    """The workspace of a mesh of V vertices and F faces and its size in bytes."""
    nbytes = _capi.lib().dvmvs_mesh_smooth_workspace_bytes(V, F)
    if nbytes == 0:
        raise ValueError(f"dvmvs::{name}: {V} vertices and {F} faces are outside what the kernels take (2^28 at most)")
    workspace = _workspace.grown("mesh_smooth", dev, nbytes, torch.int64)
    return workspace, workspace.numel() * 8


def build_rows(faces: Tensor, V: int, workspace: Tensor, nbytes: int):
    """Enqueues the rows N(v) and the boundary flags of ``faces`` (contiguous int32 [F,3]) over V >= 1 vertices into ``workspace``: the
    pair keys, ONE ``torch.sort`` of them (values only: equal keys are identical, so stability is irrelevant) and the rows entry."""
    dev, F = faces.device, int(faces.shape[0])
    pair_sorted = None
    if F:
        pair_keys = torch.empty(6 * F, dtype=torch.int64, device=dev)
        launch("dvmvs_mesh_smooth_keys", dev, ptr(faces), V, F, ptr(pair_keys), None)
        pair_sorted = torch.sort(pair_keys).values
    launch("dvmvs_mesh_smooth_rows", dev, opt_ptr(pair_sorted), V, F, ptr(workspace), nbytes)


def run_steps(verts: Tensor, F: int, workspace: Tensor, nbytes: int, iterations: int, method: str, lam: float, mu: float, boundary: str,
              packed: bool = False) -> Tensor:
    """Enqueues all steps of a call on ``verts`` (contiguous float32 [V,3], V >= 1) over the rows that ``build_rows`` left in ``workspace``,
    with ONE call of the C entry: the new positions.  ``packed``: the iterate between steps as 12-byte rows instead of 16-byte ones (the
    same bits; tools/mesh_smooth_bench.py compares the two)."""
    out = torch.empty_like(verts)
    launch("dvmvs_mesh_smooth_steps", verts.device, ptr(verts), int(verts.shape[0]), F, iterations, int(method == "taubin"), lam, mu,
           int(boundary == "fixed"), int(packed), ptr(workspace), nbytes, ptr(out))
    return out


def _normals(name, verts, faces, V, F, fallback, workspace, nbytes):
    dev = verts.device
    corner_sorted = corner_order = None
    if F:
        corner_keys = torch.empty(3 * F, dtype=torch.int32, device=dev)
        launch("dvmvs_mesh_smooth_keys", dev, ptr(faces), V, F, None, ptr(corner_keys))
        corner_sorted, corner_order = torch.sort(corner_keys, stable=True)
    out = torch.empty((V, 3), dtype=torch.float32, device=dev)
    launch("dvmvs_mesh_smooth_normals", dev, ptr(verts), V, opt_ptr(faces if F else None), F, opt_ptr(corner_sorted), opt_ptr(corner_order),
           opt_ptr(fallback), ptr(workspace), nbytes, ptr(out))
    return out


def smooth_mesh(verts: Tensor, faces: Tensor, iterations, normals: Optional[Tensor] = None, colors: Optional[Tensor] = None,
                method: str = "taubin", lam: float = 0.5, mu: float = -0.53, boundary: str = "free", recompute_normals: bool = True):
    """``dvmvs.smooth.smooth_mesh`` on the device, bit for bit: ``verts`` float32 [V,3], ``faces`` int32 [F,3], ``normals`` float32 [V,3]
    and ``colors`` uint8 [V,3] (or None) on one GPU; ``iterations`` a count, or a ``SmoothSettings`` that brings the rest.  Returns device
    tensors ``(verts', faces, normals' or None, colors or None)``; ``faces`` and ``colors`` (and ``normals`` without
    ``recompute_normals``) are copies, and no input is written.  Everything is enqueued on the current stream: the pair keys, one
    ``torch.sort`` of them, the rows, ONE C call for all the steps, and for the normals the corner keys, one stable ``torch.sort`` and the
    normals.  The whole call performs NO host read and no synchronisation: V and F do not change, so nothing has to come down to size an
    output, and there is no status to report.  Raises ``ValueError`` for the settings that ``dvmvs.smooth.smooth_settings`` refuses."""
    name = "smooth_mesh"
    if isinstance(iterations, SmoothSettings):
        iterations, method, lam, mu, boundary, recompute_normals = iterations
    iterations, method, lam, mu, boundary, recompute_normals = _settings(iterations, method, lam, mu, boundary, recompute_normals)
    verts, faces, V, F, dev = _mesh(name, verts, faces)
    if normals is not None:
        check_tensors(name, normals, label="normals", shape=(V, 3), device=dev)
        normals = normals.contiguous()
    if colors is not None:
        check_tensors(name, colors, dtype=torch.uint8, label="colors", shape=(V, 3), device=dev)
    workspace, nbytes = _workspace_of(name, dev, V, F)
    colors_out = None if colors is None else colors.clone(memory_format=torch.contiguous_format)
    if V == 0:
        return verts.clone(), faces.clone(), None if normals is None else normals.clone(), colors_out
    if iterations > 0:
        build_rows(faces, V, workspace, nbytes)
        verts_out = run_steps(verts, F, workspace, nbytes, iterations, method, lam, mu, boundary)
    else:
        verts_out = verts.clone()
    if normals is not None:
        normals = _normals(name, verts_out, faces, V, F, normals, workspace, nbytes) if recompute_normals else normals.clone()
    return verts_out, faces.clone(), normals, colors_out


def vertex_normals(verts: Tensor, faces: Tensor, fallback: Optional[Tensor] = None) -> Tensor:
    """``dvmvs.smooth.vertex_normals`` on the device, bit for bit: float32 [V,3], the area-weighted normals of the faces around every
    vertex; the row of ``fallback`` float32 [V,3] (zeros without one) where a vertex has none.  The corner keys, one stable ``torch.sort``
    and the normals are enqueued on the current stream; no host read."""
    name = "vertex_normals"
    verts, faces, V, F, dev = _mesh(name, verts, faces)
    if fallback is not None:
        check_tensors(name, fallback, label="fallback", shape=(V, 3), device=dev)
        fallback = fallback.contiguous()
    workspace, nbytes = _workspace_of(name, dev, V, F)
    if V == 0:
        return torch.empty((0, 3), dtype=torch.float32, device=dev)
    return _normals(name, verts, faces, V, F, fallback, workspace, nbytes)


def vertex_rows(faces: Tensor, V: int):
    """``dvmvs.smooth.vertex_rows`` on the device: ``(offsets int64 [V+1], neighbours int32 [E], boundary bool [V])`` as device tensors.
    For tests and tools: unlike ``smooth_mesh`` it reads E from the device (a synchronisation) to size ``neighbours``."""
    name = "vertex_rows"
    if isinstance(V, bool) or not isinstance(V, int) or not 0 <= V <= MAX_ELEMENTS:
        raise ValueError(f"dvmvs::{name}: V must be a number of vertices in [0, 2^28], got {V!r}")
    check_tensors(name, faces, dtype=torch.int32, label="faces", shape=(None, 3))
    dev, F = faces.device, int(faces.shape[0])
    faces = faces.contiguous()
    workspace, nbytes = _workspace_of(name, dev, V, F)
    offsets = torch.zeros(V + 1, dtype=torch.int64, device=dev)
    neighbours = torch.empty(6 * F, dtype=torch.int32, device=dev)
    boundary = torch.zeros(V, dtype=torch.uint8, device=dev)
    if V == 0:
        return offsets, neighbours[:0], boundary.bool()
    build_rows(faces, V, workspace, nbytes)
    launch("dvmvs_mesh_smooth_rows_export", dev, V, F, ptr(workspace), nbytes, ptr(offsets), opt_ptr(neighbours if F else None), ptr(boundary))
    return offsets, neighbours[:int(offsets[-1])], boundary.bool()

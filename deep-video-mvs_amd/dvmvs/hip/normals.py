"""Oriented normals of point clouds on the device (csrc/point_normals.hip; definition in include/dvmvs_hip.h, host form in
dvmvs/normals.py): plain functions over the C ABI and the ops package's launch plumbing, on top of the k-NN search of
``dvmvs.hip.neighbours``.  Inference-time geometry only: nothing here is registered under ``torch.ops.dvmvs`` and nothing needs
autograd."""
import math
from typing import Optional

import torch
from torch import Tensor

from dvmvs.hip import neighbours as _neighbours
from dvmvs.hip.ops._common import check_tensors, launch, ptr
from dvmvs.hip.ops.reconstruction import nearest_build
from dvmvs.normals import MAX_NEIGHBOURS, MIN_NEIGHBOURS

MAX_POINTS = 1 << 28


def _count(name, label, k):
    if isinstance(k, bool) or not isinstance(k, int) or not MIN_NEIGHBOURS <= k <= MAX_NEIGHBOURS:
        raise ValueError(f"dvmvs::{name}: {label} must be an integer in [{MIN_NEIGHBOURS}, {MAX_NEIGHBOURS}], got {k!r}")
    return k


def _viewpoints(name, N, device, viewpoints, view):
    """The checked, dense ``(viewpoints or None, V, view or None)``."""
    if viewpoints is None:
        if view is not None:
            raise ValueError(f"dvmvs::{name}: view chooses among viewpoints: it needs viewpoints")
        return None, 0, None
    check_tensors(name, viewpoints, label="viewpoints", shape=(None, 3), device=device)
    V = int(viewpoints.shape[0])
    if V < 1 or V > MAX_POINTS:
        raise ValueError(f"dvmvs::{name}: viewpoints must be float32 [V,3] with 1 <= V <= 2^28, got {tuple(viewpoints.shape)}")
    if view is None:
        if V != 1:
            raise ValueError(f"dvmvs::{name}: {V} viewpoints need view, the viewpoint of every point")
        return viewpoints.contiguous(), V, None
    check_tensors(name, view, dtype=torch.int32, label="view", shape=(N,), device=device)
    return viewpoints.contiguous(), V, view.contiguous()


def point_normals(points: Tensor, target: Tensor, index: Tensor, viewpoints: Optional[Tensor] = None, view: Optional[Tensor] = None):
    """``dvmvs.normals.point_normals`` on the device, bit for bit: ``points`` float32 [N,3], ``target`` float32 [M,3] (M >= 1) and ``index``
    int32 [N,k] (3 <= k <= 32, rows of ``neighbours.knn(points, target, k, max_distance)``; -1 and every other value outside [0, M) are
    skipped) on one GPU -> ``(normals float32 [N,3], curvature float32 [N], valid bool [N])``.  With ``viewpoints`` float32 [V,3] the
    normals are turned toward ``viewpoints[view[i]]`` (``view`` int32 [N]; without it V must be 1; an entry outside [0, V) keeps the
    canonical sign).  One launch on the current stream, nothing read by the host."""
    name = "point_normals"
    if torch.is_tensor(index) and index.dim() == 2:
        _count(name, "the slots of a row of index", int(index.shape[1]))
    check_tensors(name, points, label="points", shape=(None, 3))
    device = points.device
    check_tensors(name, target, label="target", shape=(None, 3), device=device)
    N, M = int(points.shape[0]), int(target.shape[0])
    check_tensors(name, index, dtype=torch.int32, label="index", shape=(N, None), device=device)
    k = int(index.shape[1])
    if M < 1:
        raise ValueError(f"dvmvs::{name}: the target cloud is empty")
    if N > MAX_POINTS or M > MAX_POINTS:
        raise ValueError(f"dvmvs::{name}: {N} and {M} points are outside what the kernel takes (2^28 at most)")
    viewpoints, V, view = _viewpoints(name, N, device, viewpoints, view)
    points, target, index = points.contiguous(), target.contiguous(), index.contiguous()
    normals = torch.empty((N, 3), dtype=torch.float32, device=device)
    curvature = torch.empty(N, dtype=torch.float32, device=device)
    valid = torch.empty(N, dtype=torch.uint8, device=device)
    if N > 0:
        launch("dvmvs_point_normals_fwd", device, ptr(points), N, ptr(target), M, ptr(index), k, None if viewpoints is None else ptr(viewpoints),
               V, None if view is None else ptr(view), ptr(normals), ptr(curvature), ptr(valid))
    return normals, curvature, valid.view(torch.bool)


def estimate_normals(points: Tensor, neighbours: int = 20, max_distance: float = math.inf, viewpoints: Optional[Tensor] = None,
                     view: Optional[Tensor] = None, grid: Optional[Tensor] = None):
    """``dvmvs.normals.estimate_normals`` on the device, bit for bit: the normals of a cloud float32 [N,3] from each point's ``neighbours``
    nearest points within ``max_distance``, itself among them.  One grid build (unless ``grid``, the ``ops.nearest_build`` workspace of
    the cloud, is given), one k-NN search of the cloud against itself and the normals kernel, all on the current stream; nothing read by
    the host.  ``max_distance`` also bounds the search of far outliers (``neighbours.knn``)."""
    name = "estimate_normals"
    neighbours = _count(name, "neighbours", neighbours)
    check_tensors(name, points, label="points", shape=(None, 3))
    points = points.contiguous()
    if points.shape[0] == 0:
        return (torch.zeros((0, 3), dtype=torch.float32, device=points.device), torch.zeros(0, dtype=torch.float32, device=points.device),
                torch.zeros(0, dtype=torch.bool, device=points.device))
    if grid is None:
        grid = nearest_build(points)
    _, index = _neighbours.knn(points, points, neighbours, max_distance, False, grid)
    return point_normals(points, points, index, viewpoints, view)

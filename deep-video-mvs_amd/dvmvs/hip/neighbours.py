"""The k nearest neighbours of points, neighbours within a radius and the outlier filters made of them on the device
(csrc/point_neighbours.hip; definition in include/dvmvs_hip.h, host form in dvmvs/outliers.py): plain functions over the C ABI and the
ops package's workspace and launch plumbing.  Inference-time geometry only: nothing here is registered under ``torch.ops.dvmvs`` and
nothing needs autograd."""
import math
from typing import Optional

import torch
from torch import Tensor

from dvmvs.hip import _capi
from dvmvs.hip.ops import _workspace
from dvmvs.hip.ops._common import check_tensors, launch, ptr
from dvmvs.hip.ops.reconstruction import nearest_build
from dvmvs.outliers import MAX_NEIGHBOURS, OutlierFilter, filter_settings

MAX_POINTS = 1 << 28


def _points(name, label, points, device=None):
    check_tensors(name, points, label=label, shape=(None, 3), device=device)
    return points.contiguous()


def _search(name, query, target, grid):
    """The checked clouds, the target's grid (built unless ``grid`` is it) and the scratch of one query call."""
    query = _points(name, "query", query)
    target = _points(name, "target", target, query.device)
    N, M = int(query.shape[0]), int(target.shape[0])
    if M < 1:
        raise ValueError(f"dvmvs::{name}: the target cloud is empty")
    if N > MAX_POINTS or M > MAX_POINTS:
        raise ValueError(f"dvmvs::{name}: {N} and {M} points are outside what the kernels take (2^28 at most)")
    if grid is None:
        grid = nearest_build(target)
    else:
        check_tensors(name, grid, dtype=torch.uint8, label="grid", device=query.device, contiguous=True)
        if grid.numel() < _capi.lib().dvmvs_nearest_workspace_bytes(M):
            raise ValueError(f"dvmvs::{name}: grid must be the nearest_build workspace of the target")
    scratch = None
    if N > 0:
        scratch = _workspace.grown("nearest_query", query.device, _capi.lib().dvmvs_nearest_query_workspace_bytes(N, M), torch.uint8)
    return query, target, N, M, grid, scratch


def _distance(name, label, value):
    value = float(value)
    if not value >= 0.0:
        raise ValueError(f"dvmvs::{name}: {label} must not be negative or NaN, got {value}")
    return value


def knn(query: Tensor, target: Tensor, k: int, max_distance: float = math.inf, exclude_same_index: bool = False,
        grid: Optional[Tensor] = None):
    """``dvmvs.outliers.nearest_neighbours`` on the device, bit for bit: ``query`` float32 [N,3] and ``target`` float32 [M,3] (M >= 1) on
    one GPU -> ``(dist float32 [N,k], index int32 [N,k])``, row i the k smallest ``(d2, j)`` among the targets within ``max_distance``
    (and, with ``exclude_same_index``, ``j != i``) in ascending order, missing slots ``(inf, -1)``; ``1 <= k <= 32``.  ``grid``: the
    ``ops.nearest_build`` workspace of ``target`` when the caller has it (a cloud searched against itself is then built once).  Enqueued
    on the current stream, nothing read by the host.  ``max_distance`` also bounds the work: without it a query with fewer than k
    candidates nearby, a far outlier, walks rings of cells until it has k or the grid ends."""
    name = "knn"
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_NEIGHBOURS:
        raise ValueError(f"dvmvs::{name}: k must be an integer in [1, {MAX_NEIGHBOURS}], got {k!r}")
    max_distance = _distance(name, "max_distance", max_distance)
    query, target, N, M, grid, scratch = _search(name, query, target, grid)
    dist = torch.empty((N, k), dtype=torch.float32, device=query.device)
    index = torch.empty((N, k), dtype=torch.int32, device=query.device)
    if N > 0:
        launch("dvmvs_knn_fwd", query.device, ptr(query), N, ptr(target), M, ptr(grid), ptr(scratch), scratch.numel(), k, max_distance,
               int(bool(exclude_same_index)), ptr(dist), ptr(index))
    return dist, index


def radius_count(query: Tensor, target: Tensor, radius: float, cap: int, exclude_same_index: bool = False, grid: Optional[Tensor] = None):
    """``dvmvs.outliers.radius_count`` on the device, bit for bit: int32 [N], ``min(targets within radius, cap)``; ``cap >= 1``; a query
    is left as soon as it has counted ``cap``.  ``grid`` as in ``knn``.  Enqueued on the current stream, nothing read by the host."""
    name = "radius_count"
    if isinstance(cap, bool) or not isinstance(cap, int) or not 1 <= cap < 2 ** 31:
        raise ValueError(f"dvmvs::{name}: cap must be an integer of at least 1, got {cap!r}")
    radius = _distance(name, "radius", radius)
    query, target, N, M, grid, scratch = _search(name, query, target, grid)
    count = torch.empty(N, dtype=torch.int32, device=query.device)
    if N > 0:
        launch("dvmvs_radius_count_fwd", query.device, ptr(query), N, ptr(target), M, ptr(grid), ptr(scratch), scratch.numel(), radius, cap,
               int(bool(exclude_same_index)), ptr(count))
    return count


def outlier_statistics(dist: Tensor, index: Tensor, ratio: float = 2.0):
    """The second half of ``dvmvs.outliers.statistical_outliers`` on the device, bit for bit: from ``dist`` float32 [N,k] and ``index`` int32
    [N,k] of ``knn`` -> ``(keep bool [N], mean float32 [N], stats float64 [4] = (n, mu, sigma, threshold))``.  Three launches on the
    current stream (the two sums in one workgroup, in a fixed order), nothing read by the host."""
    name = "outlier_statistics"
    check_tensors(name, dist, label="dist", shape=(None, None))
    N, k = int(dist.shape[0]), int(dist.shape[1])
    check_tensors(name, index, dtype=torch.int32, label="index", shape=(N, k), device=dist.device)
    ratio = float(ratio)
    if not 0.0 <= ratio < math.inf or not 1 <= k <= MAX_NEIGHBOURS:
        raise ValueError(f"dvmvs::{name}: ratio must be finite and not negative and k in [1, {MAX_NEIGHBOURS}], got {ratio} and {k}")
    dist, index = dist.contiguous(), index.contiguous()
    mean = torch.empty(N, dtype=torch.float32, device=dist.device)
    keep = torch.empty(N, dtype=torch.uint8, device=dist.device)
    if N == 0:
        return keep.bool(), mean, torch.zeros(4, dtype=torch.float64, device=dist.device)
    stats = torch.empty(4, dtype=torch.float64, device=dist.device)
    launch("dvmvs_outlier_statistics_fwd", dist.device, ptr(dist), ptr(index), N, k, ratio, ptr(mean), ptr(keep), ptr(stats))
    return keep.view(torch.bool), mean, stats


def statistical_outliers(points: Tensor, neighbours: int = 20, ratio: float = 2.0, max_distance: float = math.inf,
                         grid: Optional[Tensor] = None):
    """``dvmvs.outliers.statistical_outliers`` on the device, bit for bit: ``(keep bool [N], mean float32 [N], stats float64 [4])``.  One
    grid build (unless ``grid`` is given), one k-NN search of the cloud against itself and the three statistics launches; nothing read
    by the host.  ``max_distance`` bounds the search of far outliers (``knn``)."""
    points = _points("statistical_outliers", "points", points)
    if points.shape[0] == 0:
        return (torch.zeros(0, dtype=torch.bool, device=points.device), torch.zeros(0, dtype=torch.float32, device=points.device),
                torch.zeros(4, dtype=torch.float64, device=points.device))
    dist, index = knn(points, points, neighbours, max_distance, True, grid)
    return outlier_statistics(dist, index, ratio)


def radius_outliers(points: Tensor, radius: float, min_neighbours: int, grid: Optional[Tensor] = None):
    """``dvmvs.outliers.radius_outliers`` on the device, bit for bit: bool [N], True where a point has at least ``min_neighbours`` other
    points within ``radius``.  Nothing read by the host."""
    points = _points("radius_outliers", "points", points)
    if points.shape[0] == 0:
        return torch.zeros(0, dtype=torch.bool, device=points.device)
    return radius_count(points, points, radius, min_neighbours, True, grid) >= min_neighbours


def filter_outliers(cloud: Tensor, filter: OutlierFilter, return_mask: bool = False):
    """``dvmvs.outliers.filter_outliers`` on the device, bit for bit: the rows of ``cloud`` (float32 [N,C], C >= 3, xyz first) that
    ``filter`` keeps, in their original order; with ``return_mask`` also bool [N].  The searches and the statistics are enqueued on the
    current stream; the boolean index that compacts the kept rows is the one synchronisation (with both filters there are two: the
    radius filter runs on the survivors of the statistical one)."""
    name = "filter_outliers"
    neighbours, ratio, max_distance, radius, min_neighbours = filter_settings(filter)
    check_tensors(name, cloud, label="cloud", shape=(None, None))
    if cloud.shape[1] < 3:
        raise ValueError(f"dvmvs::{name}: cloud must be float32 [N,C] with C >= 3 (xyz first), got {tuple(cloud.shape)}")
    N = int(cloud.shape[0])
    keep = torch.ones(N, dtype=torch.bool, device=cloud.device)
    if neighbours is not None and N > 0:
        keep = statistical_outliers(cloud[:, :3], neighbours, ratio, max_distance)[0]
    if radius is not None and N > 0:
        survivors = torch.nonzero(keep).reshape(-1)                       # a synchronisation
        if survivors.numel() > 0:
            inner = radius_outliers(cloud[survivors, :3], radius, min_neighbours)
            keep = torch.zeros(N, dtype=torch.bool, device=cloud.device)
            keep[survivors[inner]] = True
    return (cloud[keep], keep) if return_mask else cloud[keep]

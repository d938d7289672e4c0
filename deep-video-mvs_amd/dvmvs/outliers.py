"""Outlier removal for point clouds: the step between fusing a cloud and everything done with it.  A cloud fused from predicted depth
(``dvmvs.consistency.fused_point_cloud``) carries isolated points and thin sprays along depth discontinuities; the two usual filters
remove them, the statistical one (Open3D's ``remove_statistical_outlier``) and the radius one (``remove_radius_outlier``).  Underneath
both is an exact k-nearest-neighbour search.

This module is the host definition, in numpy, importable without a GPU: a chunked brute force, usable on a few tens of thousands of
points.  ``nearest_neighbours_device``, ``statistical_outliers_device``, ``radius_outliers_device`` and ``filter_outliers_device`` are the
same on the GPU (``dvmvs.hip.neighbours``, csrc/point_neighbours.hip) and give the same bits.

Arithmetic contract, that of ``dvmvs.errors.nearest_distances``: ``d2(q, t) = (dx*dx + dy*dy) + dz*dz``, every operation an elementwise
float32 operation (each rounded, nothing fused); distances are ``sqrt(d2)``.  Coordinates must be finite."""
import math
from typing import NamedTuple, Optional

import numpy as np

MAX_NEIGHBOURS = 32
MAX_POINTS = 1 << 28                 # points the kernels take
_SUM_THREADS, _SUM_WAVE = 1024, 64   # the one workgroup of the ordered sums


def _points(name, label, points):
    points = np.ascontiguousarray(points, dtype=np.float32)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"{name}: {label} must be float32 [N,3], got {points.shape}")
    return points


def _squared_limit(name, label, value):
    """``float32(value) * float32(value)`` in float32 (inf stays inf); ``ValueError`` for a negative or NaN value."""
    try:
        value = np.float32(value)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: {label} must be a distance, got {value!r}") from None
    if not value >= 0.0:
        raise ValueError(f"{name}: {label} must not be negative or NaN, got {value}")
    with np.errstate(over="ignore"):
        return np.multiply(value, value, dtype=np.float32)


def _squared_distances(name, query, target, limit2, exclude_same_index, pairs_per_chunk):
    """Yields ``(begin, d2 float32 [n,M], candidate bool [n,M])`` for chunks of the queries."""
    query, target = _points(name, "query", query), _points(name, "target", target)
    if len(target) == 0:
        raise ValueError(f"{name}: the target cloud is empty")
    tx, ty, tz = (np.ascontiguousarray(target[:, a])[None, :] for a in range(3))
    step = max(1, int(pairs_per_chunk) // len(target))
    columns = np.arange(len(target))[None, :]
    for begin in range(0, len(query), step):
        q = query[begin:begin + step]
        with np.errstate(over="ignore"):
            dx, dy, dz = q[:, 0:1] - tx, q[:, 1:2] - ty, q[:, 2:3] - tz
            d2 = (dx * dx + dy * dy) + dz * dz
        candidate = d2 <= limit2
        if exclude_same_index:
            candidate &= columns != np.arange(begin, begin + len(q))[:, None]
        yield begin, d2, candidate


def nearest_neighbours(query, target, k, max_distance=np.inf, exclude_same_index=False, pairs_per_chunk=1 << 21):
    """The ``k`` nearest points of ``target`` [M,3] (M >= 1) for every point of ``query`` [N,3]: ``(dist float32 [N,k], index int32 [N,k])``.
    The candidates of query i are the targets j with ``d2 <= float32(max_distance) * float32(max_distance)`` (the product in float32; inf
    stays inf) and, with ``exclude_same_index``, ``j != i``: by index, for a cloud searched against itself, so a duplicate point at
    distance 0 is a neighbour.  Row i holds the k smallest candidates in ascending lexicographic order of ``(d2, j)``, the distance as
    ``sqrt(d2)``; missing slots are ``(inf, -1)``.  ``1 <= k <= 32``.  The set of the k smallest pairs does not depend on the order of
    evaluation, which is what lets a pruned search (the device's) give the same bits as this brute force.

    ``max_distance`` is also what bounds the device's work for the far outliers a filter exists for: without it a lone point is searched
    in ever wider rings of cells until it has k neighbours."""
    name = "nearest_neighbours"
    k = _neighbour_count(name, "k", k)
    limit2 = _squared_limit(name, "max_distance", max_distance)
    n = len(_points(name, "query", query))
    dist = np.full((n, k), np.inf, dtype=np.float32)
    index = np.full((n, k), -1, dtype=np.int32)
    for begin, d2, candidate in _squared_distances(name, query, target, limit2, exclude_same_index, pairs_per_chunk):
        # candidates first, then the smaller d2, then (both sorts are stable) the smaller index
        order = np.lexsort((d2, ~candidate), axis=1)[:, :k]
        rows = np.arange(len(d2))[:, None]
        found = candidate[rows, order]
        width = order.shape[1]
        dist[begin:begin + len(d2), :width] = np.where(found, np.sqrt(d2[rows, order]), np.float32(np.inf))
        index[begin:begin + len(d2), :width] = np.where(found, order, -1)
    return dist, index


def radius_count(query, target, radius, cap, exclude_same_index=False, pairs_per_chunk=1 << 21):
    """int32 [N]: ``min(number of candidates, cap)`` for every query, the candidates those of ``nearest_neighbours`` with ``max_distance =
    radius``; ``cap >= 1``.  The saturation is part of the definition, so that a search may stop as soon as it has counted ``cap``."""
    name = "radius_count"
    if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or not 1 <= int(cap) < 2 ** 31:
        raise ValueError(f"{name}: cap must be an integer of at least 1, got {cap!r}")
    limit2 = _squared_limit(name, "radius", radius)
    count = np.zeros(len(_points(name, "query", query)), dtype=np.int32)
    for begin, d2, candidate in _squared_distances(name, query, target, limit2, exclude_same_index, pairs_per_chunk):
        count[begin:begin + len(d2)] = np.minimum(np.count_nonzero(candidate, axis=1), int(cap))
    return count


def _neighbour_count(name, label, k):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= MAX_NEIGHBOURS:
        raise ValueError(f"{name}: {label} must be an integer in [1, {MAX_NEIGHBOURS}], got {k!r}")
    return int(k)


def ordered_sum(values):
    """The float64 sum of ``values`` in the fixed order of the device's one-workgroup reductions (``dvmvs_distance_metrics_fwd``), a
    function of their number alone: thread t of 1024 adds the elements t, t + 1024, ... to 0, the 64 lanes of a wave are combined by the
    xor butterfly, the 16 waves are added in order.  (Padding with zeros changes nothing: the values are never negative.)"""
    values = np.asarray(values, dtype=np.float64).reshape(-1)
    rows = -(-len(values) // _SUM_THREADS)
    padded = np.zeros(max(rows, 1) * _SUM_THREADS)
    padded[:len(values)] = values
    threads = np.zeros(_SUM_THREADS)
    for row in padded.reshape(-1, _SUM_THREADS):
        threads = threads + row
    waves = threads.reshape(_SUM_THREADS // _SUM_WAVE, _SUM_WAVE)
    lanes = np.arange(_SUM_WAVE)
    for m in (32, 16, 8, 4, 2, 1):
        waves = waves + waves[:, lanes ^ m]
    total = waves[0, 0]
    for w in range(1, len(waves)):
        total = total + waves[w, 0]
    return float(total)


def mean_neighbour_distance(dist, index):
    """float32 [N]: the float64 sum of a row's found distances (``index >= 0``) in slot order, divided by their number and rounded to
    float32 once; inf for a row without one."""
    dist, index = np.asarray(dist, dtype=np.float32), np.asarray(index)
    total = np.zeros(len(dist))
    for slot in range(dist.shape[1]):
        total = total + np.where(index[:, slot] >= 0, dist[:, slot].astype(np.float64), 0.0)
    found = np.count_nonzero(index >= 0, axis=1)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        mean = (total / np.maximum(found, 1)).astype(np.float32)
    return np.where(found > 0, mean, np.float32(np.inf)).astype(np.float32)


def outlier_statistics(mean, ratio):
    """``(keep bool [N], stats)`` from the mean neighbour distances: the second half of ``statistical_outliers``."""
    mean = np.asarray(mean, dtype=np.float32)
    valid = np.isfinite(mean)
    m = np.where(valid, mean, np.float32(0)).astype(np.float64)
    n = int(np.count_nonzero(valid))
    mu = ordered_sum(m) / n if n else 0.0
    deviation = np.where(valid, m - mu, 0.0)
    sigma = math.sqrt(ordered_sum(deviation * deviation) / (n - 1)) if n >= 2 else 0.0
    threshold = mu + float(ratio) * sigma
    return valid & (m <= threshold), np.array([n, mu, sigma, threshold], dtype=np.float64)


def _ratio(name, ratio):
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float, np.integer, np.floating)) or not 0.0 <= float(ratio) < math.inf:
        raise ValueError(f"{name}: ratio must be a finite number, not negative, got {ratio!r}")
    return float(ratio)


def statistical_outliers(points, neighbours=20, ratio=2.0, max_distance=np.inf):
    """Statistical outlier removal: ``(keep bool [N], mean float32 [N], stats float64 [4])``.  ``m_i`` is the mean distance of point i
    to its ``neighbours`` nearest other points within ``max_distance`` (``nearest_neighbours(points, points, neighbours, max_distance,
    exclude_same_index=True)``; the float64 sum of the found distances in slot order, divided by their number, rounded to float32 once; inf
    without a neighbour).  The points with a finite ``m_i`` are the valid ones, ``n`` of them; ``mu`` is their mean ``m_i``, ``sigma`` the
    sample deviation ``sqrt(sum (m_i - mu)^2 / (n - 1))`` (a second pass; 0 for ``n < 2``), both in float64 with the sums in the fixed order
    of ``ordered_sum``; ``threshold = mu + ratio * sigma``.  A point is kept when it is valid and ``float64(m_i) <= threshold``.  ``stats``
    is ``(n, mu, sigma, threshold)``; four zeros when no point is valid.

    ``max_distance`` also bounds the device's work for far outliers (``nearest_neighbours``); a point without a neighbour inside it is
    removed and left out of ``mu`` and ``sigma``."""
    name = "statistical_outliers"
    neighbours, ratio = _neighbour_count(name, "neighbours", neighbours), _ratio(name, ratio)
    points = _points(name, "points", points)
    if len(points) == 0:
        return np.zeros(0, bool), np.zeros(0, np.float32), np.zeros(4)
    dist, index = nearest_neighbours(points, points, neighbours, max_distance, exclude_same_index=True)
    mean = mean_neighbour_distance(dist, index)
    keep, stats = outlier_statistics(mean, ratio)
    return keep, mean, stats


def radius_outliers(points, radius, min_neighbours):
    """Radius outlier removal: bool [N], True where a point has at least ``min_neighbours`` other points within ``radius``
    (``radius_count(points, points, radius, cap=min_neighbours, exclude_same_index=True) >= min_neighbours``)."""
    points = _points("radius_outliers", "points", points)
    if len(points) == 0:
        return np.zeros(0, bool)
    return radius_count(points, points, radius, min_neighbours, exclude_same_index=True) >= int(min_neighbours)


class OutlierFilter(NamedTuple):
    """Which points ``filter_outliers`` keeps.  With ``neighbours`` the statistical filter (``statistical_outliers`` with ``ratio`` and
    ``max_distance``; None: unbounded), with ``radius`` and ``min_neighbours`` the radius filter (``radius_outliers``).  Both may be given:
    the statistical one runs first, the radius filter then runs on its survivors."""
    neighbours: Optional[int] = None
    ratio: float = 2.0
    max_distance: Optional[float] = None
    radius: Optional[float] = None
    min_neighbours: Optional[int] = None


def _whole(label, value, low, high):
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) or not float(value).is_integer() \
            or not low <= int(value) <= high:
        raise ValueError(f"OutlierFilter: {label} must be an integer in [{low}, {high}], got {value!r}")
    return int(value)


def filter_settings(filter):
    """``(neighbours or None, ratio, max_distance, radius or None, min_neighbours or None)`` of an ``OutlierFilter`` as the numbers that are
    used (``max_distance`` inf when not given); ``ValueError`` naming the field for a setting that is out of range, not a number, or given
    without what it belongs to, and for a filter that filters nothing."""
    if not isinstance(filter, OutlierFilter):
        raise ValueError(f"expected an OutlierFilter, got {type(filter).__name__}")
    neighbours, ratio, max_distance, radius, min_neighbours = filter
    if neighbours is not None:
        neighbours = _whole("neighbours", neighbours, 1, MAX_NEIGHBOURS)
    try:
        ratio = _ratio("OutlierFilter", ratio)
    except ValueError as e:
        raise ValueError(str(e)) from None
    if max_distance is not None:
        if neighbours is None:
            raise ValueError("OutlierFilter: max_distance bounds the search of the statistical filter: it needs neighbours")
        if isinstance(max_distance, bool) or not isinstance(max_distance, (int, float, np.integer, np.floating)) or not float(max_distance) > 0.0:
            raise ValueError(f"OutlierFilter: max_distance must be a positive distance, got {max_distance!r}")
    if (radius is None) != (min_neighbours is None):
        raise ValueError("OutlierFilter: radius and min_neighbours go together, got "
                         f"radius = {radius!r} and min_neighbours = {min_neighbours!r}")
    if radius is not None:
        if isinstance(radius, bool) or not isinstance(radius, (int, float, np.integer, np.floating)) or not 0.0 <= float(radius) < math.inf:
            raise ValueError(f"OutlierFilter: radius must be a finite distance, not negative, got {radius!r}")
        radius = float(radius)
        min_neighbours = _whole("min_neighbours", min_neighbours, 1, 2 ** 31 - 1)
    if neighbours is None and radius is None:
        raise ValueError("OutlierFilter: neither neighbours nor radius is given: nothing to filter by")
    return neighbours, ratio, math.inf if max_distance is None else float(max_distance), radius, min_neighbours


def _cloud(name, cloud):
    cloud = np.ascontiguousarray(cloud, dtype=np.float32)
    if cloud.ndim != 2 or cloud.shape[1] < 3:
        raise ValueError(f"{name}: cloud must be float32 [N,C] with C >= 3 (xyz first), got {cloud.shape}")
    return cloud


def filter_outliers(cloud, filter, return_mask=False):
    """The rows of ``cloud`` (float32 [N,C], C >= 3, xyz first: the [P,6] xyzrgb array of ``TSDFFusion.pcwrite`` passes straight through)
    that ``filter`` (an ``OutlierFilter``) keeps, in their original order; with ``return_mask`` also bool [N].  An empty cloud passes
    through."""
    neighbours, ratio, max_distance, radius, min_neighbours = filter_settings(filter)
    cloud = _cloud("filter_outliers", cloud)
    keep = np.ones(len(cloud), dtype=bool)
    if neighbours is not None and len(cloud):
        keep = statistical_outliers(cloud[:, :3], neighbours, ratio, max_distance)[0]
    if radius is not None and keep.any():
        survivors = np.flatnonzero(keep)
        keep = np.zeros(len(cloud), dtype=bool)
        keep[survivors[radius_outliers(cloud[survivors, :3], radius, min_neighbours)]] = True
    return (cloud[keep], keep) if return_mask else cloud[keep]


def nearest_neighbours_device(query, target, k, max_distance=np.inf, exclude_same_index=False):
    """``nearest_neighbours`` for device tensors (``dvmvs.hip.neighbours.knn``): the same bits, on the GPU, as device tensors; nothing is
    read by the host."""
    from dvmvs.hip import neighbours
    return neighbours.knn(query, target, k, max_distance, exclude_same_index)


def statistical_outliers_device(points, neighbours=20, ratio=2.0, max_distance=np.inf):
    """``statistical_outliers`` for a device tensor: ``(keep bool [N], mean float32 [N], stats float64 [4])`` on the GPU, the same bits;
    nothing is read by the host."""
    from dvmvs.hip import neighbours as binding
    return binding.statistical_outliers(points, neighbours, ratio, max_distance)


def radius_outliers_device(points, radius, min_neighbours):
    """``radius_outliers`` for a device tensor: bool [N] on the GPU, the same bits; nothing is read by the host."""
    from dvmvs.hip import neighbours as binding
    return binding.radius_outliers(points, radius, min_neighbours)


def filter_outliers_device(cloud, filter, return_mask=False):
    """``filter_outliers`` for a device tensor: the same rows, on the GPU.  Everything is enqueued on the current stream; the boolean
    indexing that compacts the kept rows is the one synchronisation (two with both filters)."""
    from dvmvs.hip import neighbours as binding
    return binding.filter_outliers(cloud, filter, return_mask)

"""Depth-map error metrics (numpy), as reported by the reference's evaluation (/root/reference/dvmvs/errors.py:4-28)."""
import math

import numpy as np

METRIC_NAMES = ("abs_error", "abs_relative_error", "abs_inverse_error", "squared_relative_error", "rmse",
                "ratio_125", "ratio_125_2", "ratio_125_3")


def compute_errors(gt, pred, max_depth=np.inf):
    """Eight metrics over the pixels with 0.5 <= gt <= max_depth; all-NaN when no pixel qualifies."""
    keep = (gt >= 0.5) & (gt <= max_depth)
    gt, pred = gt[keep], pred[keep]
    if gt.size == 0:
        return (np.nan,) * len(METRIC_NAMES)
    n = np.float32(gt.size)
    diff = gt - pred
    ratio = np.maximum(gt / pred, pred / gt)
    thresholds = [np.count_nonzero(ratio < 1.25 ** k) / n for k in (1, 2, 3)]
    return (np.mean(np.abs(diff)),
            np.mean(np.abs(diff) / gt),
            np.mean(np.abs(1 / gt - 1 / pred)),
            np.mean(np.square(diff) / gt),
            np.sqrt(np.mean(np.square(diff))),
            *thresholds)


def compute_errors_device(gt, pred, max_depth=np.inf):
    """``compute_errors`` for depth maps that live on the GPU, as one kernel launch (dvmvs.hip.ops.depth_errors): float32 tensors
    [H,W] -> a float32 device tensor [8]; [N,H,W] or [N,1,H,W] -> [N,8].  Same per-pixel float32 terms as ``compute_errors``, summed in
    float64 on the device; nothing is copied to the host."""
    from dvmvs.hip import ops      # (imported here: this module stays importable, and compute_errors usable, without a GPU)
    rows = ops.depth_errors(gt, pred, max_depth=max_depth)
    return rows[0] if gt.dim() == 2 else rows


RECONSTRUCTION_METRICS = ("acc", "comp", "chamfer", "precision", "recall", "fscore")


def nearest_distances(query, target, return_index=False, pairs_per_chunk=1 << 22):
    """For every point of ``query`` [N,3] the distance to the nearest point of ``target`` [M,3] (M >= 1), by chunked brute force in
    float32: ``sqrt(min_j (dx*dx + dy*dy) + dz*dz)`` with ``dx = q.x - t.x`` etc., every operation an elementwise numpy operation on float32
    arrays (each rounded, nothing fused).  With ``return_index`` also the smallest index of a nearest target (int32).  This is the
    definition the device op ``dvmvs.hip.ops.nearest_distance`` reproduces bit for bit; usable on a few tens of thousands of points."""
    query = np.ascontiguousarray(query, dtype=np.float32).reshape(-1, 3)
    target = np.ascontiguousarray(target, dtype=np.float32).reshape(-1, 3)
    if len(target) == 0:
        raise ValueError("nearest_distances: the target cloud is empty")
    tx, ty, tz = (np.ascontiguousarray(target[:, a])[None, :] for a in range(3))
    dist = np.empty(len(query), dtype=np.float32)
    index = np.empty(len(query), dtype=np.int32)
    step = max(1, int(pairs_per_chunk) // len(target))
    for begin in range(0, len(query), step):
        q = query[begin:begin + step]
        dx, dy, dz = q[:, 0:1] - tx, q[:, 1:2] - ty, q[:, 2:3] - tz
        d2 = (dx * dx + dy * dy) + dz * dz
        nearest = np.argmin(d2, axis=1)                      # the first occurrence of the minimum: the smallest index
        index[begin:begin + step] = nearest
        dist[begin:begin + step] = np.sqrt(d2[np.arange(len(q)), nearest])
    return (dist, index) if return_index else dist


def reconstruction_metrics_from_distances(dist_pred, dist_gt, threshold=0.05):
    """The six metrics from the two float32 distance arrays (prediction -> ground truth, ground truth -> prediction) and the numbers of
    distances below ``threshold``: ``(float32 [6], int64 [2])``.  Means: ``math.fsum`` in float64; every entry is formed in float64 and
    rounded to float32 once."""
    if len(dist_pred) == 0 or len(dist_gt) == 0:
        raise ValueError("reconstruction metrics of an empty point cloud are undefined")
    threshold = np.float32(threshold)
    acc = math.fsum(float(d) for d in dist_pred) / len(dist_pred)
    comp = math.fsum(float(d) for d in dist_gt) / len(dist_gt)
    counts = np.array([np.count_nonzero(dist_pred < threshold), np.count_nonzero(dist_gt < threshold)], dtype=np.int64)
    precision, recall = int(counts[0]) / len(dist_pred), int(counts[1]) / len(dist_gt)
    fscore = 2.0 * precision * recall / (precision + recall) if precision + recall > 0.0 else 0.0
    return np.array([acc, comp, (acc + comp) / 2.0, precision, recall, fscore], dtype=np.float32), counts


def compute_reconstruction_errors(pred_points, gt_points, threshold=0.05):
    """The 3-D reconstruction metrics of the Atlas / NeuralRecon / SimpleRecon evaluations between a predicted point set [N,3] and a
    ground-truth point set [M,3], float32 [6] in the order of ``RECONSTRUCTION_METRICS``:
      acc = mean distance from a predicted point to its nearest ground-truth point; comp = the same from ground truth to prediction;
      chamfer = (acc + comp) / 2; precision = share of predicted points closer than ``threshold`` (strictly) to the ground truth;
      recall = share of ground-truth points closer than ``threshold`` to the prediction; fscore = 2PR / (P + R), 0 when P + R = 0.
    The host definition: numpy, exact nearest neighbours by chunked brute force (``nearest_distances``), for a few tens of thousands of
    points.  In this package the point sets are MESH VERTICES (``TSDFVolume.score_against``): one per crossed grid edge, so their spacing
    is about one voxel and the distances are point-to-point, not point-to-surface; sampling the faces or voxel down-sampling, as some
    evaluations do, is not done here.  Raises ``ValueError`` when either set is empty."""
    pred_points = np.asarray(pred_points, dtype=np.float32).reshape(-1, 3)
    gt_points = np.asarray(gt_points, dtype=np.float32).reshape(-1, 3)
    if len(pred_points) == 0 or len(gt_points) == 0:
        raise ValueError("compute_reconstruction_errors: both point clouds must hold at least one point")
    return reconstruction_metrics_from_distances(nearest_distances(pred_points, gt_points), nearest_distances(gt_points, pred_points),
                                                 threshold)[0]


def compute_reconstruction_errors_device(pred_points, gt_points, threshold=0.05, counts=None):
    """``compute_reconstruction_errors`` for point sets that live on the GPU (float32 [N,3] and [M,3] device tensors, both non-empty):
    a float32 device tensor [6].  Two grid builds, two nearest-point queries (csrc/nearest_points.hip: the distances are the host
    function's, bit for bit) and one reduction in float64, all on the current stream; nothing is copied to the host.  ``counts``: an
    int64 [2] device tensor that receives the numbers of distances below the threshold."""
    from dvmvs.hip import ops      # (imported here: this module stays importable, and the host functions usable, without a GPU)
    for label, t in (("pred_points", pred_points), ("gt_points", gt_points)):
        if hasattr(t, "shape") and len(t.shape) == 2 and t.shape[0] == 0:
            raise ValueError(f"compute_reconstruction_errors_device: {label} is empty")
    dist_pred = ops.nearest_distance(pred_points, gt_points)
    dist_gt = ops.nearest_distance(gt_points, pred_points)
    return ops.distance_metrics(dist_pred, dist_gt, threshold, counts=counts)

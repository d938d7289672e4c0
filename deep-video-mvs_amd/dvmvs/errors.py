"""Depth-map error metrics (numpy), as reported by the reference's evaluation (/root/reference/dvmvs/errors.py:4-28)."""
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

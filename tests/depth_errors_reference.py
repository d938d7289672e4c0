"""Term-exact float64 reference of the depth-evaluation kernel (csrc/depth_errors.hip) and the case table its CPU and GPU tests share.

``reference`` computes the per-pixel float32 terms and the integer counts exactly as ``dvmvs.errors.compute_errors`` computes them on
float32 arrays (the same numpy expressions), then sums the terms in float64, divides, takes the square root for rmse and rounds once to
float32.  A float64 sum of n < 2^24 non-negative float32 terms is exact to n 2^-53 <= 2e-9 relative in the worst case and ~1e-13 in
practice, so the reference is the float32 rounding of the exact mean of compute_errors' own terms; what compute_errors adds to that is the
error of its float32 pairwise summation, which tests/test_depth_errors_reference.py bounds.
"""
import numpy as np

N_METRICS = 8
U = 2.0 ** -23           # spacing of float32 relative to the value: one rounding to nearest is within U / 2, hence within U

# name -> (H, W, why)
CASES = {
    "one_pixel": (1, 1, "n = 1, no reduction"),
    "sub_wave": (7, 13, "91 pixels, scalar path only, fewer than one wave"),
    "one_group_vec": (16, 20, "320 pixels, pure 16-byte path, under one workgroup"),
    "ragged_multi": (61, 67, "4087 pixels, four workgroups, ragged last quad; offsets 1 and 3 start frames misaligned"),
    "half_res": (128, 160, "20 workgroups: the finishing wave's lanes past the partial sums add zeros"),
    "network": (256, 320, "the product's size: 80 partial sums, more than the finishing wave's 64 lanes, so its own loop runs"),
    "chunk_loop": (513, 512, "257 chunks on the cap of 256 workgroups: workgroup 0 takes two chunks, the per-workgroup loop runs twice"),
}
MAX_DEPTHS = (np.inf, 2.0, 3.5)          # all exact in float32
BATCHES = (1, 3)
OFFSETS = (0, 1, 3)                      # elements between a 16-byte boundary and the first frame


def frame(case, k=0):
    """Seeded (gt, pred) float32 [H,W] of frame ``k`` of ``case``: gt uniform in [0, 6) with about 20 % zeros (none in the one-pixel
    frame, which is there for n = 1), pred = gt exp(N(0, 0.2)) + 0.05, arbitrary positive predictions where gt is zero."""
    H, W, _ = CASES[case]
    rng = np.random.RandomState(1000 * list(CASES).index(case) + 17 * k + 3)
    gt = rng.uniform(0.0, 6.0, (H, W))
    if case != "one_pixel":
        gt[rng.uniform(size=(H, W)) < 0.2] = 0.0
    pred = gt * np.exp(rng.normal(0.0, 0.2, (H, W))) + 0.05
    pred[gt == 0.0] = rng.uniform(0.1, 8.0, int((gt == 0.0).sum()))
    return gt.astype(np.float32), pred.astype(np.float32)


def batch(case, N):
    """(gt, pred) float32 [N,H,W]: frames 0..N-1 of the case (frame k is the same whatever N is)."""
    frames = [frame(case, k) for k in range(N)]
    return np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])


def reference(gt, pred, max_depth=np.inf):
    """(metrics float32 [8], counts int64 [4] = n and the three inlier counts) of one frame; float32 inputs."""
    gt, pred = np.asarray(gt), np.asarray(pred)
    assert gt.dtype == np.float32 and pred.dtype == np.float32 and gt.shape == pred.shape
    keep = (gt >= np.float32(0.5)) & (gt <= np.float32(max_depth))
    gt, pred = gt[keep], pred[keep]
    n = int(gt.size)
    if n == 0:
        return np.full(N_METRICS, np.nan, dtype=np.float32), np.zeros(4, dtype=np.int64)
    with np.errstate(all="ignore"):
        diff = gt - pred
        ratio = np.maximum(gt / pred, pred / gt)
        inliers = [int(np.count_nonzero(ratio < 1.25 ** k)) for k in (1, 2, 3)]
        terms = (np.abs(diff), np.abs(diff) / gt, np.abs(1 / gt - 1 / pred), np.square(diff) / gt, np.square(diff))
        assert all(t.dtype == np.float32 for t in terms) and ratio.dtype == np.float32
        means = [np.sum(t.astype(np.float64)) / n for t in terms]
        means[4] = np.sqrt(means[4])
        metrics = np.array(means + [np.float32(c) / np.float32(n) for c in inliers]).astype(np.float32)
    return metrics, np.array([n] + inliers, dtype=np.int64)


def reference_batch(gt, pred, max_depth=np.inf):
    """([N,8] float32, [N,4] int64) of [N,H,W] inputs."""
    rows = [reference(g, p, max_depth) for g, p in zip(gt, pred)]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def host_errors(gt, pred, max_depth=np.inf):
    """``compute_errors`` as a float64 [8] array (warnings of non-finite predictions silenced)."""
    from dvmvs.errors import compute_errors
    with np.errstate(all="ignore"):
        return np.array([float(v) for v in compute_errors(gt, pred, max_depth)], dtype=np.float64)


def check_against_host(got, ref_row, host_row):
    """The triangle rule for a device row against the product's host function: |m - host| <= |host - ref| + 2^-23 |ref| for every finite
    metric, identical inf / NaN pattern otherwise.  Returns the largest |m - host| / bound."""
    got, ref_row = np.asarray(got, dtype=np.float64), np.asarray(ref_row, dtype=np.float64)
    worst = 0.0
    for m, r, h in zip(got, ref_row, host_row):
        if np.isfinite(h) and np.isfinite(r):
            bound = abs(h - r) + U * abs(r)
            assert np.isfinite(m) and abs(m - h) <= bound, (m, r, h, bound)
            worst = max(worst, abs(m - h) / bound if bound > 0 else 0.0)
        else:
            assert pattern([m]) == pattern([h]), (m, r, h)
    return worst


def pattern(row):
    """'f' / '+' / '-' / 'n' per metric: finite, +inf, -inf, NaN."""
    return "".join("n" if np.isnan(v) else ("f" if np.isfinite(v) else ("+" if v > 0 else "-")) for v in np.asarray(row, dtype=np.float64))


# ---- special cases --------------------------------------------------------------------------------------------------------------------
def nothing_valid():
    """gt all zero: n = 0, eight NaNs."""
    gt, pred = frame("sub_wave")
    return np.zeros_like(gt), pred


ALL_CLIPPED_MAX_DEPTH = 0.25     # below the 0.5 m floor: no pixel passes whatever gt holds

# non_finite: ragged_multi with single predictions replaced.  Pixel (row, col) -> (gt forced to, pred forced to); gt 2.0 passes the mask
# (for max_depth = inf), gt 0.0 fails it.  Metric order: abs, abs_rel, abs_inv, sq_rel, rmse, ratio_125, ratio_125_2, ratio_125_3.
NON_FINITE = {
    # name: (edits, pattern numpy gives, inlier counts relative to the unedited frame change as stated in the test)
    "pred_zero": ([((5, 7), 2.0, 0.0)], "ff+fffff"),             # 1 / 0 = inf in the inverse error only; ratio = inf: no inlier
    "pred_negative": ([((9, 11), 2.0, -1.0)], "ffffffff"),       # all finite; both quotients negative: ratio < 1.25, an inlier to numpy
    "pred_inf": ([((20, 3), 2.0, np.inf)], "++f++fff"),          # d = -inf; 1 / inf = 0 keeps the inverse error finite
    "pred_nan": ([((33, 40), 2.0, np.nan)], "nnnnnfff"),         # NaN in all five sums; the NaN ratio is no inlier, the ratios stay finite
    "gt_nan": ([((41, 50), np.nan, 1.0)], "ffffffff"),           # a NaN gt fails the mask: n is one smaller, nothing else happens
    "masked": ([((2, 2), 0.0, 0.0), ((3, 3), 0.0, -1.0), ((4, 4), 0.0, np.inf), ((6, 6), 0.0, np.nan)], "ffffffff"),
    "together": ([((5, 7), 2.0, 0.0), ((9, 11), 2.0, -1.0), ((20, 3), 2.0, np.inf), ((33, 40), 2.0, np.nan), ((41, 50), np.nan, 1.0),
                  ((2, 2), 0.0, 0.0), ((3, 3), 0.0, -1.0), ((4, 4), 0.0, np.inf), ((6, 6), 0.0, np.nan)], "nnnnnfff"),
}


def non_finite(name):
    gt, pred = frame("ragged_multi")
    gt, pred = gt.copy(), pred.copy()
    for (row, col), g, p in NON_FINITE[name][0]:
        gt[row, col], pred[row, col] = g, p
    return gt, pred

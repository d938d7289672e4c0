"""Device time of the 3-D reconstruction metrics (csrc/nearest_points.hip) on the ``fused_scene_256`` volume of tools/tsdf_fuse_bench.py
(256^3 voxels of 1 cm): the mesh vertices of the volume with all 32 frames of that tool fused in (the "prediction") against those of the
volume with every other frame fused in (the "ground truth").

grid     ``ops.nearest_build`` and ``ops.nearest_query`` in both directions, and the whole
         ``dvmvs.errors.compute_reconstruction_errors_device`` call (two builds, two queries, one reduction): HIP events around each call
         after warm-up, [median, min, max] ms over ``--reps`` calls.
brute    the route without the op: the same float32 formula as elementwise torch operations on [chunk, M] blocks (every operation
         rounded on its own, so the distances must be EQUAL, which is checked), a min over the block's rows, both directions, and the
         metrics from torch reductions.  Timed the same way over ``--brute-reps`` calls.
Prints one JSON line; ``--out PATH`` also writes it there.

    python tools/nearest_bench.py [--reps 20] [--brute-reps 3] [--out profiles/nearest_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
for path in (os.path.join(ROOT, "deep-video-mvs_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, path)

from dvmvs.errors import RECONSTRUCTION_METRICS, compute_reconstruction_errors_device  # noqa: E402
from dvmvs.hip import ops  # noqa: E402
from tsdf_fuse_bench import frames, median_ms  # noqa: E402
from tsdf_raycast_bench import fused_scene  # noqa: E402

N_FRAMES = 32


def clouds(dev):
    """(vertices with all frames fused in, vertices with every other frame fused in): float32 [V,3] device tensors."""
    depth, rgb, _, Ks, Ps = frames(N_FRAMES, dev)
    every, other = fused_scene(dev), fused_scene(dev)
    every.integrate_frames(rgb, depth, Ks, Ps)
    other.integrate_frames(rgb[::2].contiguous(), depth[::2].contiguous(), Ks[::2].contiguous(), Ps[::2].contiguous())
    return every.vertices(), other.vertices()


def brute_distances(query, target, chunk):
    """The contract's float32 formula on [chunk, M] blocks: eager torch rounds every elementwise operation to float32."""
    tx, ty, tz = (target[:, a].contiguous()[None, :] for a in range(3))
    out = torch.empty(query.shape[0], dtype=torch.float32, device=query.device)
    for begin in range(0, query.shape[0], chunk):
        q = query[begin:begin + chunk]
        dx, dy, dz = q[:, 0:1] - tx, q[:, 1:2] - ty, q[:, 2:3] - tz
        d2 = (dx * dx + dy * dy) + dz * dz
        out[begin:begin + chunk] = d2.min(dim=1).values.sqrt()
    return out


def brute_row(pred, gt, threshold, chunk):
    a, b = brute_distances(pred, gt, chunk), brute_distances(gt, pred, chunk)
    acc, comp = a.double().mean(), b.double().mean()
    p, r = (a < threshold).double().mean(), (b < threshold).double().mean()
    f = torch.where(p + r > 0, 2 * p * r / (p + r), torch.zeros_like(p))
    return torch.stack([acc, comp, (acc + comp) / 2, p, r, f]).float(), a, b


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--brute-reps", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=512, help="queries per block of the brute force")
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pred, gt = clouds(dev)
    out = {"device": torch.cuda.get_device_name(0), "scene": "fused_scene_256", "frames": [N_FRAMES, N_FRAMES // 2], "reps": args.reps,
           "vertices": {"prediction": int(pred.shape[0]), "groundtruth": int(gt.shape[0])}, "threshold": args.threshold,
           "timing": "HIP events around each call after warm-up: [median, min, max] ms"}
    grid = {}
    for name, query, target in (("prediction_to_groundtruth", pred, gt), ("groundtruth_to_prediction", gt, pred)):
        workspace = ops.nearest_build(target)
        grid[name] = {"build_ms": median_ms(lambda: ops.nearest_build(target), args.reps),
                      "query_ms": median_ms(lambda: ops.nearest_query(query, target, workspace), args.reps)}
    grid["compute_reconstruction_errors_device_ms"] = median_ms(lambda: compute_reconstruction_errors_device(pred, gt, args.threshold), args.reps)
    row = compute_reconstruction_errors_device(pred, gt, args.threshold)
    dist_pred, dist_gt = ops.nearest_distance(pred, gt), ops.nearest_distance(gt, pred)
    out["grid"] = grid
    out["row"] = dict(zip(RECONSTRUCTION_METRICS, [float(v) for v in row.cpu()]))

    want_row, want_pred, want_gt = brute_row(pred, gt, args.threshold, args.chunk)
    brute = {"chunk": args.chunk, "pairs": 2 * int(pred.shape[0]) * int(gt.shape[0]), "reps": args.brute_reps,
             "whole_ms": median_ms(lambda: brute_row(pred, gt, args.threshold, args.chunk), args.brute_reps),
             "distances_equal_bitwise": bool(torch.equal(dist_pred.view(torch.int32), want_pred.view(torch.int32))
                                             and torch.equal(dist_gt.view(torch.int32), want_gt.view(torch.int32))),
             "row_max_abs_difference": float((row - want_row).abs().max())}
    out["brute_force_torch"] = brute
    out["brute_over_grid"] = round(brute["whole_ms"][0] / grid["compute_reconstruction_errors_device_ms"][0], 2)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    if not brute["distances_equal_bitwise"]:
        raise SystemExit("the grid search and the brute force disagree")


if __name__ == "__main__":
    main()

"""Device time of the registration (csrc/registration.hip) on the ``fused_scene_256`` clouds of tools/nearest_bench.py: the vertices of
the volume with all 32 frames fused in, displaced by 1 degree and 2 cm, are registered to the vertices of the volume with every other
frame fused in; once at the vertex counts and once at the counts their 2 cm voxel down-sampling leaves.

hip      ``dvmvs.hip.registration.icp`` with ``max_iterations=1`` (one iteration: transform, query, moments, solve) and with the default 30
         (the whole registration, as ``compute_reconstruction_errors_device(align_distance=...)`` enqueues it), on a grid built before;
         beside them ``ops.nearest_query`` of the same clouds alone and ``transform_points`` alone, to say where the time goes.
eager    the same definition without the kernels of this file: the float32 transform as torch operations, ``ops.nearest_query`` with
         indices, float64 sums by torch, the 4x4 of Horn's matrix DOWNLOADED and solved by ``torch.linalg.eigh`` on the host, the new
         transform uploaded, rmse and fitness compared on the host; one iteration and the loop to its own convergence.
HIP events around each call after warm-up, [median, min, max] ms over ``--reps`` calls.  Prints one JSON line; ``--out PATH`` writes it.

    python tools/registration_bench.py [--reps 10] [--out profiles/registration_bench.json]
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

from dvmvs.hip import ops, registration  # noqa: E402
from nearest_bench import clouds  # noqa: E402
from tsdf_fuse_bench import median_ms  # noqa: E402

MAX_DISTANCE = 0.1


def displacement():
    a = np.deg2rad(1.0)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = [0.012, -0.01, 0.0125]
    return T


def eager_iteration(source, target, grid, T):
    """One iteration in eager torch; returns (T_next or None, rmse, fitness) after ONE download of the 4x4 and the two numbers."""
    A = T[:3, :4].float()
    x, y, z = source[:, 0], source[:, 1], source[:, 2]
    moved = torch.stack([((A[r, 0] * x + A[r, 1] * y) + A[r, 2] * z) + A[r, 3] for r in range(3)], dim=1)
    dist, index = ops.nearest_query(moved, target, grid, return_index=True)
    keep = dist <= MAX_DISTANCE
    p, q = moved.double()[keep], target[index.long()].double()[keep]
    n = float(p.shape[0])
    S = p.T @ q - torch.outer(p.sum(0), q.sum(0)) / n
    d = dist.double()[keep]
    packed = torch.cat([S.reshape(-1), p.mean(0), q.mean(0), (d * d).sum().reshape(1)]).cpu()       # the download
    S, pbar, qbar, sum_d2 = packed[:9].reshape(3, 3), packed[9:12], packed[12:15], float(packed[15])
    N = torch.tensor([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                      [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                      [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], S[1, 1] - S[0, 0] - S[2, 2], S[1, 2] + S[2, 1]],
                      [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], S[2, 2] - S[0, 0] - S[1, 1]]], dtype=torch.float64)
    w, x_, y_, z_ = torch.linalg.eigh(N)[1][:, -1].tolist()
    R = torch.tensor([[1 - 2 * (y_ * y_ + z_ * z_), 2 * (x_ * y_ - w * z_), 2 * (x_ * z_ + w * y_)],
                      [2 * (x_ * y_ + w * z_), 1 - 2 * (x_ * x_ + z_ * z_), 2 * (y_ * z_ - w * x_)],
                      [2 * (x_ * z_ - w * y_), 2 * (y_ * z_ + w * x_), 1 - 2 * (x_ * x_ + y_ * y_)]], dtype=torch.float64)
    step = torch.eye(4, dtype=torch.float64)
    step[:3, :3], step[:3, 3] = R, qbar - R @ pbar
    return (step @ T.cpu()).to(source.device), (sum_d2 / n) ** 0.5, n / source.shape[0]


def eager_loop(source, target, grid, max_iterations=30, tolerance=1e-6):
    T = torch.eye(4, dtype=torch.float64, device=source.device)
    before = None
    for k in range(max_iterations):
        T_next, rmse, fitness = eager_iteration(source, target, grid, T)
        if before is not None and abs(rmse - before[0]) < tolerance and abs(fitness - before[1]) < tolerance:
            return T, k + 1
        T, before = T_next, (rmse, fitness)
    return T, max_iterations


def measure(source, target, reps):
    grid = ops.nearest_build(target, workspace=torch.empty(ops.nearest_distance_workspace(target.device, target.shape[0]).numel(),
                                                           dtype=torch.uint8, device=target.device))
    T, info = registration.icp(source, target, MAX_DISTANCE, grid=grid)
    iterations, status = int(info["iterations"]), int(info["status"])
    eager_T, eager_iterations = eager_loop(source, target, grid)
    identity = torch.eye(4, dtype=torch.float64, device=source.device)
    return {"points": {"source": int(source.shape[0]), "target": int(target.shape[0])},
            "iterations": iterations, "status": registration.STATUS_NAMES[status],
            "rmse": [round(float(v), 6) for v in info["rmse"][:iterations].cpu()],
            "hip": {"one_iteration_ms": median_ms(lambda: registration.icp(source, target, MAX_DISTANCE, max_iterations=1, grid=grid), reps),
                    "whole_30_enqueued_ms": median_ms(lambda: registration.icp(source, target, MAX_DISTANCE, grid=grid), reps),
                    "nearest_query_alone_ms": median_ms(lambda: ops.nearest_query(source, target, grid, return_index=True), reps),
                    "transform_alone_ms": median_ms(lambda: registration.transform_points(source, T), reps)},
            "eager_torch": {"iterations": eager_iterations,
                            "one_iteration_ms": median_ms(lambda: eager_iteration(source, target, grid, identity), reps),
                            "whole_ms": median_ms(lambda: eager_loop(source, target, grid), reps),
                            "max_abs_difference_of_T": float((eager_T - T).abs().max())}}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pred, gt = clouds(dev)
    away = torch.from_numpy(np.linalg.inv(displacement())).to(dev)
    pred = registration.transform_points(pred, away)
    out = {"device": torch.cuda.get_device_name(0), "scene": "fused_scene_256", "reps": args.reps, "max_distance": MAX_DISTANCE,
           "displacement": "1 degree about z and 2 cm", "timing": "HIP events around each call after warm-up: [median, min, max] ms",
           "vertices": measure(pred, gt, args.reps),
           f"voxel_{args.voxel}": measure(ops.voxel_downsample(pred, args.voxel), ops.voxel_downsample(gt, args.voxel), args.reps)}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

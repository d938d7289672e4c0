"""Device time of the point-to-plane registration (csrc/registration.hip, ``dvmvs.hip.registration.icp_plane``) beside the point-to-point
one, on the clouds of tools/registration_bench.py: the vertices of the ``fused_scene_256`` volume with all 32 frames fused in, displaced by
1 degree and 2 cm, against the vertices of the volume with every other frame fused in; once at the vertex counts and once at the counts
their 2 cm voxel down-sampling leaves.  The target's normals are estimated (``dvmvs.hip.normals.estimate_normals``, 20 neighbours, on
the grid the registration uses); that estimate is timed separately.

Per registration: the iterations to its stop and the status; ``one_iteration_ms`` (``max_iterations=1``: transform, query, moments, solve);
``whole_30_enqueued_ms`` (the default call: 30 iterations enqueued, those after the stop run their nearest query and nothing else);
``whole_needed_enqueued_ms`` (``max_iterations`` = the iterations the loop needed: what the work up to the stop costs); and
``moments_and_solve_ms``, the median of one iteration minus the medians of the nearest query alone and the transform alone.
HIP events around each call after warm-up, [median, min, max] ms over ``--reps`` calls.  Prints one JSON line; ``--out PATH`` writes it.

    python tools/registration_plane_bench.py [--reps 10] [--out profiles/registration_plane_bench.json]
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

from dvmvs.hip import normals, ops, registration  # noqa: E402
from nearest_bench import clouds  # noqa: E402
from registration_bench import MAX_DISTANCE, displacement  # noqa: E402
from tsdf_fuse_bench import median_ms  # noqa: E402

NEIGHBOURS = 20


def one(call, names, source, reps, query_ms, transform_ms):
    """The record of one registration routine; ``call(max_iterations)`` runs it."""
    T, info = call(30)
    iterations, status = int(info["iterations"]), int(info["status"])
    single = median_ms(lambda: call(1), reps)
    out = {"iterations": iterations, "status": names[status],
           "rmse": [round(float(v), 6) for v in info["rmse"][:iterations].cpu()],
           "fitness": round(float(info["fitness"][iterations - 1]), 6),
           "one_iteration_ms": single,
           "whole_30_enqueued_ms": median_ms(lambda: call(30), reps),
           "whole_needed_enqueued_ms": median_ms(lambda: call(iterations), reps),
           "moments_and_solve_ms": round(single[0] - query_ms - transform_ms, 4)}
    if "rmse_point" in info:
        out["rmse_point"] = [round(float(v), 6) for v in info["rmse_point"][:iterations].cpu()]
    return T, out


def measure(source, target, truth, reps):
    grid = ops.nearest_build(target, workspace=torch.empty(ops.nearest_distance_workspace(target.device, target.shape[0]).numel(),
                                                           dtype=torch.uint8, device=target.device))
    target_normals, _, valid = normals.estimate_normals(target, NEIGHBOURS, grid=grid)
    query = median_ms(lambda: ops.nearest_query(source, target, grid, return_index=True), reps)
    identity = torch.eye(4, dtype=torch.float64, device=source.device)
    transform = median_ms(lambda: registration.transform_points(source, identity), reps)
    point_T, point = one(lambda k: registration.icp(source, target, MAX_DISTANCE, max_iterations=k, grid=grid), registration.STATUS_NAMES,
                         source, reps, query[0], transform[0])
    plane_T, plane = one(lambda k: registration.icp_plane(source, target, target_normals, MAX_DISTANCE, max_iterations=k, grid=grid),
                         registration.PLANE_STATUS_NAMES, source, reps, query[0], transform[0])
    point["max_abs_difference_from_displacement"] = float((point_T - truth).abs().max())
    plane["max_abs_difference_from_displacement"] = float((plane_T - truth).abs().max())
    return {"points": {"source": int(source.shape[0]), "target": int(target.shape[0])},
            "targets_with_normal": int(valid.sum()),
            "nearest_query_alone_ms": query, "transform_alone_ms": transform,
            "estimate_normals_ms": median_ms(lambda: normals.estimate_normals(target, NEIGHBOURS, grid=grid), reps),
            "point_to_point": point, "point_to_plane": plane}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pred, gt = clouds(dev)
    truth = torch.from_numpy(displacement()).to(dev)
    pred = registration.transform_points(pred, torch.from_numpy(np.linalg.inv(displacement())).to(dev))
    out = {"device": torch.cuda.get_device_name(0), "scene": "fused_scene_256", "reps": args.reps, "max_distance": MAX_DISTANCE,
           "displacement": "1 degree about z and 2 cm", "normal_neighbours": NEIGHBOURS,
           "timing": "HIP events around each call after warm-up: [median, min, max] ms",
           "vertices": measure(pred, gt, truth, args.reps),
           f"voxel_{args.voxel}": measure(ops.voxel_downsample(pred, args.voxel), ops.voxel_downsample(gt, args.voxel), truth, args.reps)}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

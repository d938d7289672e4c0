"""Device time of meshing an oriented point cloud (``dvmvs.hip.implicit.mesh_points``; csrc/implicit_surface.hip) stage by stage, on the
vertex cloud of the ``fused_scene_256`` volume of tools/tsdf_fuse_bench.py (256^3 voxels of 1 cm, all 32 frames fused in) with the normals
``estimate_normals`` gives it (20 neighbours within 5 cm, oriented toward one viewpoint), at ``--voxel`` 2 cm and ``--radius`` 5 cm.

stages   band (fill and kernel), nonzero (the candidate list, a host read), nodes, search (``neighbours.knn`` of the candidate nodes against
         the cloud, its grid built beforehand), values (fills and kernel), marching cubes (in index space), trim (flags, compaction,
         re-indexing), nearest (``ops.nearest_query`` of the vertices and the gathers of normals): HIP events around each stage after
         warm-up, [median, min, max] ms over ``--reps`` calls, every stage on the outputs of the one before.  ``whole`` is
         ``mesh_points`` itself, which also finds the cloud's box, builds the grid of the cloud and moves the vertices to world space.
counts   dense (all nodes of the grid), candidate (marked by the band), searched_with_a_candidate (of those, the nodes whose row is not
         empty: what the band would mark if it marked balls instead of cubes), valid.
torch    the same definition in eager torch on the device, from the same candidate list and the same rows: the node positions in float32,
         the gathers of the [A,k,3] points and normals, the slot loop in float64 (eager torch rounds every elementwise operation on its
         own, so the bits must be the kernel's: ``equal_bits``), the scatter.  The search is the project's kernel in both routes.
band     the alternative that was tried and is not shipped, in torch: one scatter of every point's nearest node into the mask, then a
         dilation (``max_pool3d``) by the reach plus the half voxel of the scatter; it must mark a superset of what the cubes mark.
Prints one JSON line; ``--out PATH`` also writes it there.

    python tools/implicit_surface_bench.py [--reps 20] [--torch-reps 3] [--out profiles/implicit_surface_bench.json]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
for path in (os.path.join(ROOT, "deep-video-mvs_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, path)

from dvmvs import implicit as host  # noqa: E402
from dvmvs.hip import implicit, neighbours, normals, ops  # noqa: E402
from dvmvs.hip.ops._common import launch, ptr  # noqa: E402
from dvmvs.tsdf import marching_cubes  # noqa: E402
from nearest_bench import clouds  # noqa: E402
from point_outliers_bench import timed_ms  # noqa: E402


def values_stage(nodes, cloud, cloud_normals, index, k, radius, min_neighbours, linear, dims):
    volume = torch.full(dims, float(radius), dtype=torch.float32, device=cloud.device)
    valid = torch.zeros(dims, dtype=torch.uint8, device=cloud.device)
    launch("dvmvs_implicit_values_fwd", cloud.device, ptr(nodes), int(nodes.shape[0]), ptr(cloud), ptr(cloud_normals), int(cloud.shape[0]),
           ptr(index), k, float(radius), min_neighbours, ptr(linear), volume.numel(), ptr(volume), ptr(valid))
    return volume, valid.view(torch.bool)


def torch_values(linear, cloud, cloud_normals, index, origin, voxel, dims, radius, min_neighbours):
    """The definition in eager torch: ``(volume, valid)`` from the candidate list and its rows."""
    dev = cloud.device
    X, Y, Z = dims
    ijk = torch.stack([linear // (Y * Z), (linear // Z) % Y, linear % Z], dim=1)
    nodes = ijk.float() * torch.tensor(float(voxel), dtype=torch.float32, device=dev)
    nodes = nodes + torch.as_tensor(origin, dtype=torch.float32, device=dev)
    M = cloud.shape[0]
    inside = (index >= 0) & (index < M)
    j = index.clamp(0, M - 1).long()
    has_normal = (cloud_normals != 0).any(dim=1)
    x, p, n = nodes.double(), cloud.double(), cloud_normals.double()
    h2 = float(radius) * float(radius)
    num = torch.zeros(linear.shape[0], dtype=torch.float64, device=dev)
    den, used = torch.zeros_like(num), torch.zeros(linear.shape[0], dtype=torch.int32, device=dev)
    for slot in range(index.shape[1]):
        js = j[:, slot]
        ok = inside[:, slot] & has_normal[js]
        e = x - p[js]
        d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        t = 1.0 - d2 / h2
        t = torch.where(t < 0, torch.zeros_like(t), t)
        w = (t * t) * t
        ns = n[js]
        s = (ns[:, 0] * e[:, 0] + ns[:, 1] * e[:, 1]) + ns[:, 2] * e[:, 2]
        num = torch.where(ok, num + w * s, num)
        den = torch.where(ok, den + w, den)
        used = used + ok.int()
    good = (used >= min_neighbours) & (den > 0)
    volume = torch.full((X * Y * Z,), float(radius), dtype=torch.float32, device=dev)
    valid = torch.zeros(X * Y * Z, dtype=torch.bool, device=dev)
    volume[linear[good]] = (num[good] / den[good]).float()
    valid[linear[good]] = True
    return volume.reshape(dims), valid.reshape(dims)


def dilated_band(cloud, origin, voxel, dims, radius):
    """The alternative band: the nearest node of every point, dilated by the kernel's reach plus the half voxel between a point and its
    nearest node (the coordinate term of the reach taken at the cloud's largest coordinate)."""
    dev = cloud.device
    v, r = float(voxel), float(radius)
    o = torch.as_tensor(origin, dtype=torch.float64, device=dev)
    g = (cloud.double() - o) / v
    largest = float(cloud.abs().max()) + float(np.abs(origin).max())
    reach = (r * (1.0 + 2.0 ** -20) + 2.0 ** -22 * (largest + r) + 2.0 ** -62) / v + 2.0 ** -20
    R = int(math.floor(reach + 0.5))
    near = torch.round(g).long()
    limit = torch.tensor(dims, device=dev)
    near = torch.minimum(torch.maximum(near, torch.zeros_like(near) - R), limit - 1 + R)      # outside by more than R marks nothing anyway
    padded = torch.zeros((1, 1, dims[0] + 2 * R, dims[1] + 2 * R, dims[2] + 2 * R), dtype=torch.float16, device=dev)
    padded[0, 0, near[:, 0] + R, near[:, 1] + R, near[:, 2] + R] = 1.0
    mask = torch.nn.functional.max_pool3d(padded, kernel_size=2 * R + 1, stride=1)
    return (mask[0, 0] > 0).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--radius", type=float, default=0.05)
    ap.add_argument("--neighbours", type=int, default=32)
    ap.add_argument("--min-neighbours", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cloud = clouds(dev)[0].contiguous()
    N = int(cloud.shape[0])
    viewpoint = (cloud.mean(dim=0) + torch.tensor([0.0, 0.0, 3.0], device=dev)).reshape(1, 3).contiguous()
    cloud_normals, _, normal_valid = normals.estimate_normals(cloud, 20, 0.05, viewpoint)
    cloud_normals = cloud_normals.contiguous()
    voxel, radius, k, min_n = np.float32(args.voxel), np.float32(args.radius), args.neighbours, args.min_neighbours
    origin, dims = host.grid_for(cloud.cpu().numpy(), voxel, radius)
    grid = ops.nearest_build(cloud, workspace=torch.empty(ops.nearest_distance_workspace(dev, N).numel(), dtype=torch.uint8, device=dev))
    reps = args.reps
    out = {"device": torch.cuda.get_device_name(0), "scene": "fused_scene_256", "points": N, "points_with_a_normal": int(normal_valid.sum()),
           "reps": reps, "settings": {"voxel": float(voxel), "radius": float(radius), "neighbours": k, "min_neighbours": min_n,
                                      "normals": "estimate_normals(cloud, 20, 0.05, one viewpoint)"},
           "grid": {"origin": [float(o) for o in origin], "dims": list(dims)},
           "timing": "HIP events around each stage after warm-up: [median, min, max] ms", "stage_ms": {}}
    stage = out["stage_ms"]

    mask = implicit.band(cloud, origin, voxel, dims, radius)
    stage["band"] = timed_ms(lambda: implicit.band(cloud, origin, voxel, dims, radius), reps)
    linear = torch.nonzero(mask.reshape(-1)).reshape(-1)
    stage["nonzero"] = timed_ms(lambda: torch.nonzero(mask.reshape(-1)).reshape(-1), reps)
    A = int(linear.numel())
    if A > 1 << 20:
        out["note"] = f"{A} candidates: mesh_points searches them in chunks of 2^20; the stages below run them as one chunk"
    nodes = implicit.node_positions(linear, origin, voxel, dims)
    stage["nodes"] = timed_ms(lambda: implicit.node_positions(linear, origin, voxel, dims), reps)
    index = neighbours.knn(nodes, cloud, k, float(radius), False, grid)[1]
    stage["search"] = timed_ms(lambda: neighbours.knn(nodes, cloud, k, float(radius), False, grid), reps)
    volume, valid = values_stage(nodes, cloud, cloud_normals, index, k, radius, min_n, linear, dims)
    stage["values"] = timed_ms(lambda: values_stage(nodes, cloud, cloud_normals, index, k, radius, min_n, linear, dims), reps)
    verts_index, faces, _, _ = marching_cubes(volume, 0.0, None, (0.0, 0.0, 0.0), 1.0)
    stage["marching_cubes"] = timed_ms(lambda: marching_cubes(volume, 0.0, None, (0.0, 0.0, 0.0), 1.0), reps)
    trimmed = implicit.trim_mesh(verts_index, faces, valid)
    stage["trim"] = timed_ms(lambda: implicit.trim_mesh(verts_index, faces, valid), reps)
    verts = trimmed[0] * torch.tensor(float(voxel), device=dev) + torch.as_tensor(origin, device=dev)

    def nearest_stage():
        found = ops.nearest_query(verts, cloud, grid, return_index=True)[1].long()
        return cloud_normals[found]

    stage["nearest"] = timed_ms(nearest_stage, reps)
    out["stage_sum_ms"] = round(sum(v[0] for v in stage.values()), 4)
    out["stage_share_percent"] = {name: round(100.0 * v[0] / out["stage_sum_ms"], 1) for name, v in stage.items()}
    out["whole_ms"] = timed_ms(lambda: implicit.mesh_points(cloud, cloud_normals, float(voxel), float(radius), k, min_n), reps)
    mesh = implicit.mesh_points(cloud, cloud_normals, float(voxel), float(radius), k, min_n)
    out["counts"] = {"dense": int(np.prod(dims)), "candidate": A, "searched_with_a_candidate": int((index[:, 0] >= 0).sum()),
                     "valid": int(valid.sum()), "vertices_before_trim": int(verts_index.shape[0]), "faces_before_trim": int(faces.shape[0]),
                     "vertices": int(mesh[0].shape[0]), "faces": int(mesh[1].shape[0])}
    same_mesh = torch.equal(mesh[0], verts) and torch.equal(mesh[1], trimmed[1])
    out["whole_equals_stages"] = bool(same_mesh)

    eager = timed_ms(lambda: torch_values(linear, cloud, cloud_normals, index, origin, voxel, dims, radius, min_n), args.torch_reps, warm=1)
    want = torch_values(linear, cloud, cloud_normals, index, origin, voxel, dims, radius, min_n)
    equal = torch.equal(want[0].view(torch.int32), volume.view(torch.int32)) and torch.equal(want[1], valid)
    out["eager_torch"] = {"reps": args.torch_reps, "nodes_and_values_ms": eager, "equal_bits": bool(equal),
                          "over_kernels": round(eager[0] / (stage["nodes"][0] + stage["values"][0]), 1)}

    other = dilated_band(cloud, origin, voxel, dims, radius)
    out["band_alternative"] = {"what": "scatter of nearest nodes and max_pool3d dilation, eager torch",
                               "ms": timed_ms(lambda: dilated_band(cloud, origin, voxel, dims, radius), reps),
                               "marked": int(other.sum()), "superset_of_the_cubes": bool((other >= mask).all())}
    ok = equal and same_mesh and out["band_alternative"]["superset_of_the_cubes"]
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    if not ok:
        raise SystemExit("the kernels and the torch formulation disagree")


if __name__ == "__main__":
    main()

"""Device time of the k-nearest-neighbour search, the radius count and the outlier filter (csrc/point_neighbours.hip) on the vertex
cloud of the ``fused_scene_256`` volume of tools/tsdf_fuse_bench.py (256^3 voxels of 1 cm, all 32 frames fused in), and on the same cloud
with ``--isolated`` points scattered through a box three times its size: the far outliers the filter exists for.

grid     ``neighbours.knn`` of the cloud against itself (``exclude_same_index``) for k = 8, 20, 32, with ``--max-distance`` and unbounded,
         on a prebuilt grid; ``neighbours.radius_count``; and the whole ``dvmvs.outliers.filter_outliers_device`` call (grid build, search,
         statistics, compaction): HIP events around each call after warm-up, [median, min, max] ms over ``--reps`` calls.
torch    the route without the kernels, timed in the same run: the same float32 formula as elementwise torch operations on [chunk, N]
         blocks (every operation rounded on its own), the own index and the pairs beyond the limit set to inf, ``topk`` of the block's
         rows; the radius count as a sum over the same blocks; the statistical filter from those distances with torch reductions.  The
         distances and the counts must be EQUAL bit for bit and the kept points the same, which is checked (``topk`` does not order
         equal distances by index, so the indices are compared only where a row's distances are all different).
kdtree   if scipy imports: ``cKDTree`` on the host in float64, the download of the cloud included; its distances must agree with the
         float32 ones within the contract's 4 * 2^-24 relative error.
Prints one JSON line; ``--out PATH`` also writes it there.

    python tools/point_outliers_bench.py [--reps 20] [--torch-reps 2] [--out profiles/point_outliers_bench.json]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
for path in (os.path.join(ROOT, "deep-video-mvs_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, path)

from dvmvs.hip import neighbours, ops  # noqa: E402
from dvmvs.outliers import OutlierFilter, filter_outliers_device  # noqa: E402
from nearest_bench import clouds  # noqa: E402

KS = (8, 20, 32)


def timed_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(end))
    return [round(float(np.median(times)), 4), round(float(np.min(times)), 4), round(float(np.max(times)), 4)]


def with_isolated_points(cloud, count, seed=0):
    """The cloud with ``count`` points scattered uniformly through a box three times its size around it, at random places of the array."""
    generator = torch.Generator(device="cpu").manual_seed(seed)
    lo, hi = cloud.min(dim=0).values, cloud.max(dim=0).values
    centre, half = (lo + hi) / 2, (hi - lo) / 2
    extra = centre + (torch.rand((count, 3), generator=generator).to(cloud.device) * 2 - 1) * 3 * half
    both = torch.cat([cloud, extra.float()])
    return both[torch.randperm(both.shape[0], generator=generator).to(cloud.device)].contiguous()


def torch_blocks(cloud, limit, chunk):
    """Yields ``(begin, d2 [n,N])`` with the own index and the pairs beyond the limit at inf: eager torch rounds every operation to float32."""
    tx, ty, tz = (cloud[:, a].contiguous()[None, :] for a in range(3))
    limit2 = torch.tensor(limit, dtype=torch.float32, device=cloud.device) ** 2
    for begin in range(0, cloud.shape[0], chunk):
        q = cloud[begin:begin + chunk]
        dx, dy, dz = q[:, 0:1] - tx, q[:, 1:2] - ty, q[:, 2:3] - tz
        d2 = (dx * dx + dy * dy) + dz * dz
        d2 = torch.where(d2 <= limit2, d2, torch.full_like(d2, math.inf))
        rows = torch.arange(q.shape[0], device=cloud.device)
        d2[rows, begin + rows] = math.inf
        yield begin, d2


def torch_knn(cloud, k, limit, chunk):
    dist = torch.empty((cloud.shape[0], k), dtype=torch.float32, device=cloud.device)
    index = torch.empty((cloud.shape[0], k), dtype=torch.int64, device=cloud.device)
    for begin, d2 in torch_blocks(cloud, limit, chunk):
        best = torch.topk(d2, k, dim=1, largest=False, sorted=True)
        dist[begin:begin + d2.shape[0]] = best.values.sqrt()
        index[begin:begin + d2.shape[0]] = best.indices
    return dist, index


def torch_radius_count(cloud, radius, cap, chunk):
    count = torch.empty(cloud.shape[0], dtype=torch.int32, device=cloud.device)
    for begin, d2 in torch_blocks(cloud, radius, chunk):
        count[begin:begin + d2.shape[0]] = (d2 < math.inf).sum(dim=1).clamp(max=cap)
    return count


def torch_statistical(cloud, k, ratio, limit, chunk):
    dist, _ = torch_knn(cloud, k, limit, chunk)
    found = dist < math.inf
    mean = (torch.where(found, dist.double(), torch.zeros_like(dist, dtype=torch.float64)).sum(dim=1) / found.sum(dim=1).clamp(min=1)).float()
    mean = torch.where(found.any(dim=1), mean, torch.full_like(mean, math.inf))
    valid = torch.isfinite(mean)
    m = mean.double()[valid]
    threshold = m.mean() + ratio * m.std(unbiased=True)
    return cloud[valid & (mean.double() <= threshold)]


def measure(cloud, args):
    dev = cloud.device
    N = int(cloud.shape[0])
    grid = ops.nearest_build(cloud, workspace=torch.empty(ops.nearest_distance_workspace(dev, N).numel(), dtype=torch.uint8, device=dev))
    out = {"points": N, "grid_build_ms": timed_ms(lambda: ops.nearest_build(cloud), args.reps)}
    statistical = OutlierFilter(neighbours=20, ratio=args.ratio, max_distance=args.max_distance)
    both = statistical._replace(radius=args.radius, min_neighbours=args.min_neighbours)
    for name, limit in (("bounded", args.max_distance), ("unbounded", math.inf)):
        out[f"knn_{name}_ms"] = {f"k{k}": timed_ms(lambda: neighbours.knn(cloud, cloud, k, limit, True, grid), args.reps) for k in KS}
    out["radius_count_ms"] = timed_ms(lambda: neighbours.radius_count(cloud, cloud, args.radius, args.min_neighbours, True, grid), args.reps)
    out["filter_statistical_ms"] = timed_ms(lambda: filter_outliers_device(cloud, statistical), args.reps)
    out["filter_both_ms"] = timed_ms(lambda: filter_outliers_device(cloud, both), args.reps)
    kept = filter_outliers_device(cloud, statistical)
    out["kept"] = {"statistical": int(kept.shape[0]), "both": int(filter_outliers_device(cloud, both).shape[0])}

    eager = {"chunk": args.chunk, "reps": args.torch_reps}
    equal = True
    for k in KS:
        eager[f"knn_bounded_k{k}_ms"] = timed_ms(lambda: torch_knn(cloud, k, args.max_distance, args.chunk), args.torch_reps, warm=1)
        dist, index = neighbours.knn(cloud, cloud, k, args.max_distance, True, grid)
        want_dist, want_index = torch_knn(cloud, k, args.max_distance, args.chunk)
        untied = ((dist[:, 1:] != dist[:, :-1]).all(dim=1) & (dist < math.inf).all(dim=1))
        equal = equal and torch.equal(dist.view(torch.int32), want_dist.view(torch.int32)) and torch.equal(index[untied].long(), want_index[untied])
        eager[f"rows_without_ties_k{k}"] = int(untied.sum())
    eager["radius_count_ms"] = timed_ms(lambda: torch_radius_count(cloud, args.radius, args.min_neighbours, args.chunk), args.torch_reps, warm=1)
    equal = equal and torch.equal(neighbours.radius_count(cloud, cloud, args.radius, args.min_neighbours, True, grid),
                                  torch_radius_count(cloud, args.radius, args.min_neighbours, args.chunk))
    eager["filter_statistical_ms"] = timed_ms(lambda: torch_statistical(cloud, 20, args.ratio, args.max_distance, args.chunk), args.torch_reps, warm=1)
    equal = equal and torch.equal(kept, torch_statistical(cloud, 20, args.ratio, args.max_distance, args.chunk))
    eager["results_equal"] = bool(equal)
    out["eager_torch"] = eager
    out["torch_over_kernels"] = {"knn_bounded_k20": round(eager["knn_bounded_k20_ms"][0] / out["knn_bounded_ms"]["k20"][0], 1),
                                 "radius_count": round(eager["radius_count_ms"][0] / out["radius_count_ms"][0], 1),
                                 "filter_statistical": round(eager["filter_statistical_ms"][0] / out["filter_statistical_ms"][0], 1)}
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        out["kdtree_host"] = None
        return out, equal
    times = []
    for _ in range(args.torch_reps):
        torch.cuda.synchronize()
        start = time.perf_counter()
        host = cloud.cpu().numpy().astype(np.float64)
        tree_dist, _ = cKDTree(host).query(host, k=21, distance_upper_bound=args.max_distance)
        times.append(1000.0 * (time.perf_counter() - start))
    dist = neighbours.knn(cloud, cloud, 20, args.max_distance, True, grid)[0].cpu().numpy().astype(np.float64)
    # the tree's first column is the point itself or a duplicate of it: the 20 others are what is left without ONE zero
    tree_dist = np.sort(tree_dist, axis=1)[:, 1:]
    finite = np.isfinite(dist) & np.isfinite(tree_dist)
    agree = bool((np.isfinite(dist) == np.isfinite(tree_dist)).mean() > 0.9999
                 and (np.abs(dist - tree_dist)[finite] <= 4.0 * 2.0 ** -24 * tree_dist[finite] + 1e-12).all())
    out["kdtree_host"] = {"knn_bounded_k20_with_download_ms": [round(float(np.median(times)), 2), round(min(times), 2), round(max(times), 2)],
                          "distances_within_the_float32_bound": agree}
    return out, equal and agree


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=512, help="queries per block of the torch formulation")
    ap.add_argument("--isolated", type=int, default=200, help="isolated points added for the second cloud")
    ap.add_argument("--max-distance", type=float, default=0.05)
    ap.add_argument("--ratio", type=float, default=2.0)
    ap.add_argument("--radius", type=float, default=0.03)
    ap.add_argument("--min-neighbours", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    surface = clouds(dev)[0].contiguous()
    out = {"device": torch.cuda.get_device_name(0), "scene": "fused_scene_256", "reps": args.reps,
           "settings": {"neighbours": 20, "ratio": args.ratio, "max_distance": args.max_distance, "radius": args.radius,
                        "min_neighbours": args.min_neighbours, "isolated": args.isolated},
           "timing": "HIP events around each call after warm-up: [median, min, max] ms"}
    ok = True
    for name, cloud in (("surface", surface), ("surface_with_isolated_points", with_isolated_points(surface, args.isolated))):
        out[name], equal = measure(cloud, args)
        ok = ok and equal
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    if not ok:
        raise SystemExit("the kernels and the torch formulation (or the KD-tree) disagree")


if __name__ == "__main__":
    main()

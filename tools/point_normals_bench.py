"""Device time of the point-normals kernel (csrc/point_normals.hip) and of the whole ``estimate_normals`` call on the vertex cloud of the
``fused_scene_256`` volume of tools/tsdf_fuse_bench.py (256^3 voxels of 1 cm, all 32 frames fused in), for k = 8, 20, 32 neighbours within
``--max-distance``, oriented toward one viewpoint.

kernel   ``dvmvs.hip.normals.point_normals`` on rows found beforehand, and ``estimate_normals`` whole (grid build, k-NN search, normals):
         HIP events around each call after warm-up, [median, min, max] ms over ``--reps`` calls.
torch    the route without the kernel, timed in the same run: the same definition as eager float64 torch on the device, the gather of
         the [N,k,3] neighbourhoods by index, the anchored moments as masked sums, ``torch.linalg.eigh`` of the [N,3,3] covariances, the
         orientation.  ``eigh`` is another algorithm, so the normals are compared by angle, not bits: sin(angle) <= 1e-6 wherever both
         call the point valid and the relative gap between the two smallest eigenvalues exceeds 1e-6 (float64 perturbs an eigenvector by
         about 1e-10 at that gap; the float32 rounding of the output is 6e-8), which is asserted.
numpy    ``dvmvs.normals.point_normals`` on the host at k = 20, the download of the cloud and of the rows included; its outputs must EQUAL
         the kernel's bit for bit.
index    with ``--index-variants`` and the tools-only library (``make -C deep-video-mvs_amd/csrc tuning``; DVMVS_HIP_LIB pointing at
         it): the kernel with its index rows staged through LDS (the product) and read directly, interleaved rounds in this process.
Prints one JSON line; ``--out PATH`` also writes it there.

    python tools/point_normals_bench.py [--reps 20] [--torch-reps 3] [--out profiles/point_normals_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
for path in (os.path.join(ROOT, "deep-video-mvs_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, path)

from dvmvs import normals as host  # noqa: E402
from dvmvs.hip import neighbours, normals, ops  # noqa: E402
from nearest_bench import clouds  # noqa: E402
from point_outliers_bench import timed_ms  # noqa: E402

KS = (8, 20, 32)


def torch_normals(points, index, viewpoint):
    """``(normals float64 [N,3], valid bool [N], gap float64 [N])`` by eager torch: the definition's moments, ``eigh`` for the 3x3."""
    inside = (index >= 0) & (index < points.shape[0])
    nb = points.double()[index.clamp(0, points.shape[0] - 1).long()]                   # [N,k,3]
    first = inside.int().argmax(dim=1)
    anchor = nb[torch.arange(points.shape[0], device=points.device), first]
    e = (nb - anchor[:, None, :]) * inside[:, :, None]
    n = inside.sum(dim=1).clamp(min=1).double()
    m = e.sum(dim=1) / n[:, None]
    C = torch.einsum("nkc,nkd->ncd", e, e) / n[:, None, None] - m[:, :, None] * m[:, None, :]
    w, v = torch.linalg.eigh(C)
    normal = v[:, :, 0]
    valid = (inside.sum(dim=1) >= host.MIN_NEIGHBOURS) & (w.sum(dim=1) > 0)
    d = (normal * (viewpoint.double() - points.double())).sum(dim=1)
    normal = torch.where((d < 0)[:, None], -normal, normal)
    gap = (w[:, 1] - w[:, 0]) / w[:, 2].clamp(min=1e-300)
    return normal, valid, gap


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--max-distance", type=float, default=0.05)
    ap.add_argument("--index-variants", action="store_true", help="compare the staged and the direct index reads (needs the tuning library)")
    ap.add_argument("--rounds", type=int, default=5, help="interleaved rounds of --index-variants")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cloud = clouds(dev)[0].contiguous()
    N = int(cloud.shape[0])
    viewpoint = (cloud.mean(dim=0) + torch.tensor([0.0, 0.0, 3.0], device=dev)).reshape(1, 3).contiguous()
    grid = ops.nearest_build(cloud, workspace=torch.empty(ops.nearest_distance_workspace(dev, N).numel(), dtype=torch.uint8, device=dev))
    out = {"device": torch.cuda.get_device_name(0), "scene": "fused_scene_256", "points": N, "reps": args.reps,
           "settings": {"max_distance": args.max_distance, "viewpoints": 1},
           "timing": "HIP events around each call after warm-up: [median, min, max] ms",
           "kernel_ms": {}, "knn_ms": {}, "estimate_normals_ms": {}, "valid": {}, "eager_torch": {"reps": args.torch_reps}}
    ok = True
    rows = {}
    for k in KS:
        index = neighbours.knn(cloud, cloud, k, args.max_distance, False, grid)[1]
        rows[k] = index
        out["knn_ms"][f"k{k}"] = timed_ms(lambda: neighbours.knn(cloud, cloud, k, args.max_distance, False, grid), args.reps)
        out["kernel_ms"][f"k{k}"] = timed_ms(lambda: normals.point_normals(cloud, cloud, index, viewpoint), args.reps)
        out["estimate_normals_ms"][f"k{k}"] = timed_ms(lambda: normals.estimate_normals(cloud, k, args.max_distance, viewpoint), args.reps)
        got, _, valid = normals.point_normals(cloud, cloud, index, viewpoint)
        out["valid"][f"k{k}"] = int(valid.sum())
        eager = out["eager_torch"]
        eager[f"k{k}_ms"] = timed_ms(lambda: torch_normals(cloud, index, viewpoint), args.torch_reps, warm=1)
        want, want_valid, gap = torch_normals(cloud, index, viewpoint)
        both = valid & want_valid & (gap > 1e-6)
        sine = torch.linalg.cross(got.double(), want).norm(dim=1)[both]
        eager[f"k{k}_compared"] = int(both.sum())
        eager[f"k{k}_validity_differs"] = int((valid != want_valid).sum())
        eager[f"k{k}_max_sine"] = float(sine.max()) if sine.numel() else 0.0
        ok = ok and eager[f"k{k}_max_sine"] <= 1e-6 and eager[f"k{k}_compared"] >= 0.99 * int(valid.sum())
    out["eager_torch"]["normals_agree"] = bool(ok)
    out["torch_over_kernel"] = {f"k{k}": round(out["eager_torch"][f"k{k}_ms"][0] / out["kernel_ms"][f"k{k}"][0], 1) for k in KS}
    # bytes the kernel must move at least once: the rows, the outputs, and the cloud (gathered; counted once)
    out["kernel_min_bytes"] = {f"k{k}": N * (4 * k + 12 + 12 + 4 + 1 + 12) for k in KS}
    out["kernel_gb_per_s_of_min_bytes"] = {f"k{k}": round(out["kernel_min_bytes"][f"k{k}"] / out["kernel_ms"][f"k{k}"][0] / 1e6, 1) for k in KS}

    times = []
    for _ in range(2):
        torch.cuda.synchronize()
        start = time.perf_counter()
        points_host, index_host, view_host = cloud.cpu().numpy(), rows[20].cpu().numpy(), viewpoint.cpu().numpy()
        want = host.point_normals(points_host, points_host, index_host, view_host)
        times.append(1000.0 * (time.perf_counter() - start))
    got = normals.point_normals(cloud, cloud, rows[20], viewpoint)
    equal = all(g.cpu().numpy().tobytes() == w.tobytes() for g, w in zip(got, want))
    out["numpy_host"] = {"k20_with_download_ms": [round(float(np.median(times)), 1), round(min(times), 1), round(max(times), 1)],
                         "equal_bits": bool(equal)}
    out["numpy_over_kernel_k20"] = round(out["numpy_host"]["k20_with_download_ms"][0] / out["kernel_ms"]["k20"][0], 1)
    ok = ok and equal

    if args.index_variants:
        variants = {"staged": {}, "direct": {}}
        same = True
        for k in KS:
            samples = {name: [] for name in variants}
            for _ in range(args.rounds):
                for name in variants:
                    os.environ["DVMVS_POINT_NORMALS_INDEX"] = name
                    samples[name].append(timed_ms(lambda: normals.point_normals(cloud, cloud, rows[k], viewpoint), args.reps)[0])
            results = {}
            for name in variants:
                os.environ["DVMVS_POINT_NORMALS_INDEX"] = name
                results[name] = normals.point_normals(cloud, cloud, rows[k], viewpoint)
                variants[name][f"k{k}_ms"] = [round(float(np.median(samples[name])), 4), round(min(samples[name]), 4)]
            same = same and all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(results["staged"], results["direct"]))
        os.environ.pop("DVMVS_POINT_NORMALS_INDEX")
        library = os.environ.get("DVMVS_HIP_LIB")
        out["index_read"] = {"library": os.path.relpath(library, ROOT) if library else None, "rounds": args.rounds,
                             "timing": "[median, min] over the rounds of each round's median ms", **variants, "equal_bits": bool(same)}
        if variants["staged"]["k20_ms"] == variants["direct"]["k20_ms"] and not os.environ.get("DVMVS_HIP_LIB"):
            out["index_read"]["note"] = "the product library has the staged read only: point DVMVS_HIP_LIB at the tuning library"
        ok = ok and same
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    if not ok:
        raise SystemExit("the kernel and the torch formulation (or the host form) disagree")


if __name__ == "__main__":
    main()

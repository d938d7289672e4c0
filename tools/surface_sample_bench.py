"""Device time of the point sets the 3-D metrics are taken between (csrc/surface_sample.hip) on the ``fused_scene_256`` volumes of
tools/nearest_bench.py (256^3 voxels of 1 cm; all 32 frames fused in = the "prediction", every other frame = the "ground truth").

ops      ``ops.surface_sample`` of the prediction's mesh at the density that yields about ``--points`` samples, ``ops.voxel_downsample`` of
         that cloud at ``--voxel``, and the whole ``TSDFVolume.score_against(other, sample_density=..., voxel=...)`` (two marching cubes,
         two samplings, two down-samplings, two grid builds, two queries, one reduction): HIP events around each call after warm-up,
         [median, min, max] ms over ``--reps`` calls.  Each op reads one size on the host per call; that wait is inside the time.
eager    the same definitions as eager torch operations on the device: float64 cross products, ``cumsum``, ``searchsorted``, gathers and
         float32 blends for the samples; ``unique`` and ``index_add_`` for the voxels.  Checked first: the samples must be EQUAL bit for
         bit; the voxels' keys and populations must be equal, and their means may differ in the last float32 bit, since ``index_add_``
         adds in the order its atomics arrive in (how many do is reported).  Timed the same way.
vertices the score without the new arguments (``score_against(other)``: what the program did before), for scale.
Prints one JSON line; ``--out PATH`` also writes it there.

    python tools/surface_sample_bench.py [--reps 20] [--out profiles/surface_sample_bench.json]
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
from nearest_bench import N_FRAMES  # noqa: E402
from tsdf_fuse_bench import frames, median_ms  # noqa: E402
from tsdf_raycast_bench import fused_scene  # noqa: E402


def volumes(dev):
    depth, rgb, _, Ks, Ps = frames(N_FRAMES, dev)
    every, other = fused_scene(dev), fused_scene(dev)
    every.integrate_frames(rgb, depth, Ks, Ps)
    other.integrate_frames(rgb[::2].contiguous(), depth[::2].contiguous(), Ks[::2].contiguous(), Ps[::2].contiguous())
    return every, other


def lowbias32(x):
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    return x ^ (x >> 16)


def eager_areas(verts, faces):
    """int64 [F]: the quantised areas (every face of a marching-cubes mesh names vertices that exist: no validity test here)."""
    tri = faces.long()
    a, b, c = (verts[tri[:, j]].double() for j in range(3))
    e1, e2 = b - a, c - a
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    n2 = (cx * cx + cy * cy) + cz * cz
    return torch.round(torch.sqrt(n2) * 0.5 * 4294967296.0).long()


def eager_surface_sample(verts, faces, density, seed=0):
    cum = torch.cumsum(eager_areas(verts, faces), 0)
    D = max(int(np.rint(4294967296.0 / density)), 1)
    total = int(cum[-1])                                              # the one host read
    N = 0 if total <= D >> 1 else (total - (D >> 1) - 1) // D + 1
    k = torch.arange(N, dtype=torch.int64, device=verts.device)
    face = torch.searchsorted(cum, k * D + (D >> 1), right=True)
    h1 = (k * 0xC13FA9A9 + lowbias32(seed)) & 0xffffffff
    h2 = (k * 0x91E10DA5 + lowbias32((seed + 1) & 0xffffffff)) & 0xffffffff
    u = (h1 >> 8).float() * 2.0 ** -24
    v = (h2 >> 8).float() * 2.0 ** -24
    fold = u + v > 1.0
    u, v = torch.where(fold, 1.0 - u, u), torch.where(fold, 1.0 - v, v)
    tri = faces.long()[face]
    a, b, c = verts[tri[:, 0]], verts[tri[:, 1]], verts[tri[:, 2]]
    return (a + u[:, None] * (b - a)) + v[:, None] * (c - a)


def eager_voxel_downsample(points, voxel):
    inv = float(np.float32(1.0 / voxel))
    cells = ((points - points.min(dim=0).values) * inv).to(torch.int64)
    keys = (cells[:, 0] << 42) | (cells[:, 1] << 21) | cells[:, 2]
    unique, inverse, counts = torch.unique(keys, return_inverse=True, return_counts=True)
    sums = torch.zeros((unique.shape[0], 3), dtype=torch.float64, device=points.device).index_add_(0, inverse, points.double())
    return (sums / counts[:, None].double()).float(), counts


def eager_score(every, other, density, voxel, threshold):
    sides = []
    for vol in (every, other):
        verts, faces = vol.mesh_tensors()
        sides.append(eager_voxel_downsample(eager_surface_sample(verts, faces, density), voxel)[0])
    return compute_reconstruction_errors_device(sides[0], sides[1], threshold)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--points", type=float, default=1e6, help="samples the density is chosen for")
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    every, other = volumes(dev)
    verts, faces = every.mesh_tensors()
    area = float(eager_areas(verts, faces).sum()) / 4294967296.0
    density = float(round(args.points / area))
    out = {"device": torch.cuda.get_device_name(0), "scene": "fused_scene_256", "frames": [N_FRAMES, N_FRAMES // 2], "reps": args.reps,
           "mesh": {"vertices": int(verts.shape[0]), "faces": int(faces.shape[0]), "area_m2": round(area, 3)}, "density": density,
           "voxel": args.voxel, "threshold": args.threshold,
           "timing": "HIP events around each call after warm-up, the call's host read included: [median, min, max] ms"}

    # the eager route gives the same results
    points, want_points = ops.surface_sample(verts, faces, density), eager_surface_sample(verts, faces, density)
    down, population = ops.voxel_downsample(points, args.voxel, return_counts=True)
    want_down, want_population = eager_voxel_downsample(points, args.voxel)
    same_shape = down.shape == want_down.shape
    checks = {"samples_equal_bitwise": bool(points.shape == want_points.shape and torch.equal(points.view(torch.int32), want_points.view(torch.int32))),
              "voxel_populations_equal": bool(same_shape and torch.equal(population.long(), want_population)),
              "voxel_means_not_bitwise_equal": int((down.view(torch.int32) != want_down.view(torch.int32)).sum()) if same_shape else -1,
              "voxel_means_max_abs_difference": float((down - want_down).abs().max()) if same_shape else float("nan")}
    row = every.score_against(other, args.threshold, sample_density=density, voxel=args.voxel)
    want_row = eager_score(every, other, density, args.voxel, args.threshold)
    checks["row_max_abs_difference"] = float((row - want_row).abs().max())
    out["eager_route_checks"] = checks
    out["points"] = {"samples": int(points.shape[0]), "voxels": int(down.shape[0])}
    out["row"] = dict(zip(RECONSTRUCTION_METRICS, [float(v) for v in row.cpu()]))
    plain = every.score_against(other, args.threshold)
    out["row_on_vertices"] = dict(zip(RECONSTRUCTION_METRICS, [float(v) for v in plain.cpu()]))

    out["ops"] = {"surface_sample_ms": median_ms(lambda: ops.surface_sample(verts, faces, density), args.reps),
                  "voxel_downsample_ms": median_ms(lambda: ops.voxel_downsample(points, args.voxel), args.reps),
                  "score_against_ms": median_ms(lambda: every.score_against(other, args.threshold, sample_density=density, voxel=args.voxel),
                                                args.reps)}
    out["eager"] = {"surface_sample_ms": median_ms(lambda: eager_surface_sample(verts, faces, density), args.reps),
                    "voxel_downsample_ms": median_ms(lambda: eager_voxel_downsample(points, args.voxel), args.reps),
                    "score_against_ms": median_ms(lambda: eager_score(every, other, density, args.voxel, args.threshold), args.reps)}
    out["vertices_only"] = {"score_against_ms": median_ms(lambda: every.score_against(other, args.threshold), args.reps)}
    out["eager_over_ops"] = {k: round(out["eager"][k][0] / out["ops"][k][0], 2) for k in out["ops"]}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    if not (checks["samples_equal_bitwise"] and checks["voxel_populations_equal"]) or not checks["voxel_means_max_abs_difference"] < 1e-6:
        raise SystemExit("the ops and the eager route disagree")


if __name__ == "__main__":
    main()

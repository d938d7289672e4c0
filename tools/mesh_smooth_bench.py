"""Device time of mesh smoothing (csrc/mesh_smooth.hip) on the mesh of the ``fused_scene_256`` volume of tools/marching_cubes_bench.py.

rows      the rows N(v) and the boundary flags: the pair keys, the one sort, ``dvmvs_mesh_smooth_rows``.
steps     ``dvmvs_mesh_smooth_steps`` alone over rows that are built: Laplacian at 1, 10 and 100 iterations, with the iterate between steps
          as 16-byte rows (the product) and as 12-byte rows; a step's time is the slope between 10 and 100.
normals   ``dvmvs.hip.smooth.vertex_normals``: the corner keys, the stable sort, the normals.
whole     ``dvmvs.hip.smooth.smooth_mesh`` with normals and colours, Taubin at 10 iterations: every launch, both sorts, the allocations and
          the copies of faces and colours.
eager     the same definition in eager torch on the device: ``index_add_`` of float64 positions over the directed pair list (built once,
          outside the timing; its build is timed on its own), the division and the update, 20 steps.  Its sums are atomic and in another
          order, so its positions differ from the definition's: the largest difference is reported.
numpy     ``dvmvs.smooth.smooth_mesh`` on the host with the download of the mesh and the upload of the result.
fan       one vertex with 10^5 neighbours next to the scene's mesh size of ordinary rows: the serial walk of one lane.
HIP events around each call after warm-up: [median, min, max] ms over ``--reps`` calls.  Prints one JSON line; ``--out PATH`` writes it.

    python tools/mesh_smooth_bench.py [--reps 20] [--out profiles/mesh_smooth_bench.json]
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

from dvmvs.hip import smooth  # noqa: E402
from dvmvs.hip.ops._common import launch, ptr  # noqa: E402
from dvmvs.smooth import SmoothSettings, smooth_mesh, step_factors  # noqa: E402
from dvmvs.tsdf import marching_cubes  # noqa: E402
from marching_cubes_bench import fused_scene  # noqa: E402
from tsdf_fuse_bench import median_ms  # noqa: E402

TAUBIN = SmoothSettings(10)
STEP_COUNTS = (1, 10, 100)


def eager_pairs(faces, V):
    """``(a int64 [E], b int64 [E], count float64 [V])``: the distinct directed pairs of the counting faces, in eager torch."""
    index = faces.long()
    a, b, c = index[:, 0], index[:, 1], index[:, 2]
    counting = ((index >= 0) & (index < V)).all(dim=1) & (a != b) & (b != c) & (a != c)
    a, b, c = a[counting], b[counting], c[counting]
    keys = torch.unique(torch.cat([(a << 32) | b, (b << 32) | a, (b << 32) | c, (c << 32) | b, (c << 32) | a, (a << 32) | c]))
    first, second = keys >> 32, keys & 0xffffffff
    return first, second, torch.zeros(V, dtype=torch.float64, device=faces.device).index_add_(0, first, torch.ones_like(first, dtype=torch.float64))


def eager_steps(verts, pairs, factors):
    first, second, count = pairs
    moves = count > 0
    divisor = torch.where(moves, count, torch.ones_like(count))[:, None]
    x = verts
    for s in factors:
        x64 = x.double()
        mean = torch.zeros_like(x64).index_add_(0, first, x64[second]) / divisor
        x = torch.where(moves[:, None], (x64 + s * (mean - x64)).float(), x)
    return x


def fan_mesh(dev, rim, ordinary):
    """A hub with ``rim`` neighbours, and a strip of ``ordinary`` further vertices with rows of four."""
    angle = 2.0 * np.pi * np.arange(rim) / rim
    verts = np.concatenate([[[0.0, 0.0, 0.4]], np.stack([np.cos(angle), np.sin(angle), np.zeros(rim)], axis=1)])
    i = np.arange(rim)
    faces = np.stack([np.zeros(rim, dtype=np.int64), 1 + i, 1 + (i + 1) % rim], axis=1)
    j = np.arange(ordinary)
    strip = np.stack([(j // 2) * 0.01, (j % 2) * 0.01 + 2.0, np.zeros(ordinary)], axis=1)
    f = np.arange(ordinary - 2)
    strip_faces = np.stack([f, f + 1, f + 2], axis=1) + len(verts)
    return (torch.from_numpy(np.concatenate([verts, strip]).astype(np.float32)).to(dev),
            torch.from_numpy(np.concatenate([faces, strip_faces]).astype(np.int32)).to(dev))


def steps_only(verts, faces, reps, packed, counts=STEP_COUNTS):
    V, F = int(verts.shape[0]), int(faces.shape[0])
    workspace, nbytes = smooth._workspace_of("mesh_smooth_bench", verts.device, V, F)
    smooth.build_rows(faces, V, workspace, nbytes)
    out = {}
    for n in counts:
        out[f"laplacian_{n}_ms"] = median_ms(lambda: smooth.run_steps(verts, F, workspace, nbytes, n, "laplacian", 0.5, -0.53, "free", packed), reps)
    low, high = counts[-2], counts[-1]
    out[f"per_step_us_slope_{low}_to_{high}"] = round(1000.0 * (out[f"laplacian_{high}_ms"][0] - out[f"laplacian_{low}_ms"][0]) / (high - low), 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    reps = args.reps
    dev = torch.device("cuda:0")
    tsdf, color = fused_scene(dev)
    verts, faces, normals, colors = marching_cubes(tsdf, 0.0, color, np.array([-1.28, -1.28, 0.0], dtype=np.float32), 0.01)
    V, F = int(verts.shape[0]), int(faces.shape[0])
    offsets, neighbours, boundary = smooth.vertex_rows(faces, V)
    lengths = (offsets[1:] - offsets[:-1]).cpu().numpy()
    out = {"device": torch.cuda.get_device_name(0), "scene": "fused_scene_256", "reps": reps, "vertices": V, "faces": F,
           "timing": "[median, min, max] ms: HIP events around each call after 3 warm-up calls",
           "row_length_mean": round(float(lengths.mean()), 3), "row_length_max": int(lengths.max()), "row_entries": int(neighbours.shape[0]),
           "boundary_vertices": int(boundary.sum()), "positions_16_byte_bytes": 16 * V}
    workspace, nbytes = smooth._workspace_of("mesh_smooth_bench", dev, V, F)
    out["rows_build_ms"] = median_ms(lambda: smooth.build_rows(faces, V, workspace, nbytes), reps)
    pair_keys = torch.empty(6 * F, dtype=torch.int64, device=dev)
    launch("dvmvs_mesh_smooth_keys", dev, ptr(faces), V, F, ptr(pair_keys), None)
    out["rows_build_sort_alone_ms"] = median_ms(lambda: torch.sort(pair_keys), reps)
    out["steps_16_byte_positions"] = steps_only(verts, faces, reps, packed=False)
    out["steps_12_byte_positions"] = steps_only(verts, faces, reps, packed=True)
    out["vertex_normals_ms"] = median_ms(lambda: smooth.vertex_normals(verts, faces, normals), reps)
    out["whole_call_taubin_10_ms"] = median_ms(lambda: smooth.smooth_mesh(verts, faces, TAUBIN, normals, colors), reps)
    out["whole_call_taubin_10_without_normals_ms"] = median_ms(lambda: smooth.smooth_mesh(verts, faces, TAUBIN), reps)
    result = smooth.smooth_mesh(verts, faces, TAUBIN, normals, colors)

    factors = step_factors(TAUBIN.iterations, TAUBIN.method, TAUBIN.lam, TAUBIN.mu)
    out["eager_torch_pair_list_ms"] = median_ms(lambda: eager_pairs(faces, V), reps)
    pairs = eager_pairs(faces, V)
    out["eager_torch_20_steps_ms"] = median_ms(lambda: eager_steps(verts, pairs, factors), reps)
    out["hip_20_steps_ms"] = median_ms(lambda: smooth.run_steps(verts, F, workspace, nbytes, 10, "taubin", 0.5, -0.53, "free"), reps)
    out["eager_torch_max_abs_position_difference_m"] = float((eager_steps(verts, pairs, factors) - result[0]).abs().max())

    def on_host():
        mesh = [t.cpu().numpy() for t in (verts, faces, normals, colors)]
        return [torch.from_numpy(a).to(dev) for a in smooth_mesh(mesh[0], mesh[1], TAUBIN, mesh[2], mesh[3])]

    out["numpy_on_the_host_with_transfers_ms"] = median_ms(on_host, max(2, reps // 10))
    out["numpy_equals_the_call"] = bool(all(torch.equal(a, b) for a, b in zip(on_host(), result)))

    rim = 100000
    fan_verts, fan_faces = fan_mesh(dev, rim, V)
    out["fan"] = {"hub_neighbours": rim, "vertices": int(fan_verts.shape[0]), "faces": int(fan_faces.shape[0]),
                  "steps": steps_only(fan_verts, fan_faces, max(2, reps // 4), packed=False, counts=(1, 5))}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

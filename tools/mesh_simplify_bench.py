"""Device time of mesh simplification (csrc/mesh_simplify.hip) on the mesh of the ``fused_scene_256`` volume of
tools/marching_cubes_bench.py, at cells of 4 cm and 8 cm, and what the smaller mesh costs downstream.

whole     ``dvmvs.hip.simplify.simplify_mesh`` with normals and colours (quadric and average): every launch, the four stable sorts, the one
          host read, the allocations.
stages    the same sequence enqueued stage by stage with HIP events between the stages (one pass, medians per stage): the voxel keys and
          runs of the vertices with their sort, ``keys``, the sort of the incidences, the two sorts of the canonical triples with
          ``pair_keys`` between them, ``count``, the host read, ``emit``.
eager     the cell means and the face mapping of the same definition in eager torch on the device (``unique`` with inverse,
          ``index_add_`` in float64, boolean masks); no quadric, no duplicate removal.  Its float64 sums are atomic, so its means may differ
          from the definition's in the last bit: the largest difference is reported, not assumed zero.
quality   ``compute_reconstruction_errors_device`` of the simplified against the unsimplified mesh, both sampled on their faces.
after     ``render_mesh`` of 16 views and ``surface_sample`` on the mesh before and after.
long_run  the fan of tests/simplify_reference.py scaled to 10^5 incidences in one cell next to ordinary cells: the serial walk of one thread.
HIP events around each call after warm-up: [median, min, max] ms over ``--reps`` calls.  Prints one JSON line; ``--out PATH`` writes it.

    python tools/mesh_simplify_bench.py [--reps 20] [--out profiles/mesh_simplify_bench.json]
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

import simplify_reference as sr  # noqa: E402
from dvmvs.errors import compute_reconstruction_errors_device  # noqa: E402
from dvmvs.hip import _capi, ops, simplify  # noqa: E402
from dvmvs.hip.ops import _workspace  # noqa: E402
from dvmvs.hip.ops._common import launch, ptr  # noqa: E402
from dvmvs.simplify import quadric_ranks  # noqa: E402
from dvmvs.tsdf import marching_cubes, render_mesh  # noqa: E402
from marching_cubes_bench import fused_scene  # noqa: E402
from tsdf_fuse_bench import median_ms  # noqa: E402

CELLS = (0.04, 0.08)
STAGES = ("voxel_keys", "sort_vertex_keys", "voxel_runs", "keys", "sort_incidences", "sort_third", "pair_keys", "sort_pair", "count", "host_read",
          "emit")
DENSITY = 2000.0
K = np.array([[300.0, 0, 159.5], [0, 300.0, 127.5], [0, 0, 1.0]])
H, W = 256, 320


def staged(verts, faces, normals, colors, voxel, reps):
    """{stage: [median, min, max] ms} of ``simplify.simplify_mesh``'s own sequence (quadric, with attributes and indices)."""
    dev = verts.device
    V, F = int(verts.shape[0]), int(faces.shape[0])
    lib = _capi.lib()
    inv, limit = float(np.float32(1.0 / voxel)), float(np.float32(voxel))
    voxel_ws = _workspace.grown("voxel_downsample", dev, lib.dvmvs_voxel_downsample_workspace_bytes(V), torch.uint8)
    ws = _workspace.grown("mesh_simplify", dev, lib.dvmvs_mesh_simplify_workspace_bytes(V, F), torch.int64)
    nbytes = ws.numel() * 8
    times = {s: [] for s in STAGES}
    for rep in range(reps + 3):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(STAGES) + 1)]
        ev[0].record()
        keys = torch.empty(V, dtype=torch.int64, device=dev)
        launch("dvmvs_voxel_keys", dev, ptr(verts), V, inv, ptr(voxel_ws), voxel_ws.numel(), ptr(keys))
        ev[1].record()
        sorted_keys, sorted_index = torch.sort(keys, stable=True)
        ev[2].record()
        voxel_counts = torch.empty(2, dtype=torch.int64, device=dev)
        launch("dvmvs_voxel_downsample_count", dev, ptr(verts), V, ptr(sorted_keys), ptr(sorted_index), ptr(voxel_ws), voxel_ws.numel(),
               ptr(voxel_counts))
        ev[3].record()
        inc, third, pair = (torch.empty(3 * F, dtype=torch.int32, device=dev), torch.empty(F, dtype=torch.int32, device=dev),
                            torch.empty(F, dtype=torch.int64, device=dev))
        launch("dvmvs_mesh_simplify_keys", dev, ptr(faces), V, F, ptr(sorted_index), ptr(voxel_ws), ptr(voxel_counts), ptr(ws), nbytes, ptr(inc),
               ptr(third), ptr(pair))
        ev[4].record()
        inc_sorted, inc_order = torch.sort(inc, stable=True)
        ev[5].record()
        _, third_order = torch.sort(third, stable=True)
        ev[6].record()
        pair_in_order = torch.empty(F, dtype=torch.int64, device=dev)
        launch("dvmvs_mesh_simplify_pair_keys", dev, ptr(pair), ptr(third_order), F, ptr(pair_in_order))
        ev[7].record()
        pair_sorted, pair_order = torch.sort(pair_in_order, stable=True)
        ev[8].record()
        counts = torch.empty(3, dtype=torch.int64, device=dev)
        launch("dvmvs_mesh_simplify_count", dev, ptr(verts), ptr(normals), ptr(colors), V, ptr(faces), F, limit, 0, ptr(sorted_index), ptr(voxel_ws),
               ptr(voxel_counts), ptr(inc_sorted), ptr(inc_order), ptr(third), ptr(third_order), ptr(pair_sorted), ptr(pair_order), ptr(ws), nbytes,
               ptr(counts))
        ev[9].record()
        V_out, F_out, status = (int(c) for c in counts.cpu())
        assert status == 0
        ev[10].record()
        out = (torch.empty((V_out, 3), dtype=torch.float32, device=dev), torch.empty((F_out, 3), dtype=torch.int32, device=dev),
               torch.empty((V_out, 3), dtype=torch.float32, device=dev), torch.empty((V_out, 3), dtype=torch.uint8, device=dev),
               torch.empty(V, dtype=torch.int32, device=dev), torch.empty(F_out, dtype=torch.int32, device=dev))
        launch("dvmvs_mesh_simplify_emit", dev, V, F, ptr(ws), nbytes, V_out, F_out, *(ptr(t) for t in out))
        ev[11].record()
        torch.cuda.synchronize()
        if rep >= 3:
            for i, s in enumerate(STAGES):
                times[s].append(ev[i].elapsed_time(ev[i + 1]))
    result = {s: [round(float(np.median(t)), 4), round(float(np.min(t)), 4), round(float(np.max(t)), 4)] for s, t in times.items()}
    total = sum(r[0] for r in result.values())
    sorts = sum(result[s][0] for s in ("sort_incidences", "sort_third", "sort_pair"))
    result["sum_of_medians_ms"] = round(total, 4)
    result["three_face_sorts_share"] = round(sorts / total, 4)
    result["all_four_sorts_share"] = round((sorts + result["sort_vertex_keys"][0]) / total, 4)
    return result, out


def eager_means_and_mapping(verts, faces, voxel):
    """(cell means float32 [M,3], mapped proper faces int64 [F'',3], the cell of every vertex int64 [V]) in eager torch."""
    inv = float(np.float32(1.0 / voxel))
    cells = ((verts - verts.min(dim=0).values) * inv).to(torch.int32).long()
    keys = (cells[:, 0] << 42) | (cells[:, 1] << 21) | cells[:, 2]
    _, inverse, counts = torch.unique(keys, return_inverse=True, return_counts=True)
    sums = torch.zeros((counts.shape[0], 3), dtype=torch.float64, device=verts.device).index_add_(0, inverse, verts.double())
    means = (sums / counts[:, None].double()).float()
    index = faces.long()
    valid = ((index >= 0) & (index < verts.shape[0])).all(dim=1)
    mapped = inverse[index.clamp(0, verts.shape[0] - 1)]
    proper = valid & (mapped[:, 0] != mapped[:, 1]) & (mapped[:, 1] != mapped[:, 2]) & (mapped[:, 0] != mapped[:, 2])
    return means, mapped[proper], inverse


def views(n=16):
    poses = np.tile(np.eye(4), (n, 1, 1))
    poses[:, 0, 3] = np.linspace(-0.3, 0.3, n)
    poses[:, 1, 3] = 0.1 * np.sin(np.arange(n))
    return poses


def downstream(verts, faces, reps):
    poses = views()
    return {"render_mesh_16_views_ms": median_ms(lambda: render_mesh(verts, faces, K, poses, H, W), reps),
            "surface_sample_ms": median_ms(lambda: ops.surface_sample(verts, faces, DENSITY), reps)}


def measure(mesh, voxel, reps):
    verts, faces, normals, colors = mesh
    out = {"cell_m": voxel}
    results = {}
    for contraction in ("quadric", "average"):
        results[contraction] = simplify.simplify_mesh(verts, faces, voxel, normals, colors, contraction, return_index=True)
        out[f"whole_call_{contraction}_ms"] = median_ms(
            lambda: simplify.simplify_mesh(verts, faces, voxel, normals, colors, contraction, return_index=True), reps)
    quadric, average = results["quadric"], results["average"]
    out.update(vertices_out=int(quadric[0].shape[0]), faces_out=int(quadric[1].shape[0]))
    out["stages_quadric_ms"], staged_out = staged(verts, faces, normals, colors, voxel, reps)
    out["stages_equal_the_call"] = bool(all(torch.equal(a, b) for a, b in zip(staged_out, list(quadric[:4]) + list(quadric[4]))))
    means, mapped, inverse = eager_means_and_mapping(verts, faces, voxel)
    out["eager_torch_means_and_mapping_ms"] = median_ms(lambda: eager_means_and_mapping(verts, faces, voxel), reps)
    # the eager means are those of ALL cells; the call's are the cells that kept a face: compare through vertex_cluster
    cluster = quadric[4][0].long()
    used = cluster >= 0
    out["eager_means_max_abs_difference_m"] = float((means[inverse[used]] - average[0][cluster[used]]).abs().max())
    out["eager_proper_faces"] = int(mapped.shape[0])
    ranks = np.bincount(quadric_ranks(verts.cpu().numpy(), faces.cpu().numpy(), voxel), minlength=4)
    out["rank_histogram_all_cells_0_to_3"] = [int(r) for r in ranks]
    for contraction, result in results.items():
        row = compute_reconstruction_errors_device(result[0], verts, 0.01, pred_faces=result[1], gt_faces=faces, sample_density=DENSITY)
        row = row.cpu().numpy()
        out[f"against_unsimplified_{contraction}"] = {"accuracy_m": float(row[0]), "completeness_m": float(row[1]), "chamfer_m": float(row[2])}
    out["downstream_before"] = downstream(verts, faces, reps)
    out["downstream_after_quadric"] = downstream(quadric[0], quadric[1], reps)
    return out


def long_run(dev, reps, incidences=100000):
    case = sr.long_run(incidences // 3)
    t = {k: torch.from_numpy(np.array(v)).to(dev) for k, v in case.items() if isinstance(v, np.ndarray)}
    call = lambda contraction: simplify.simplify_mesh(t["verts"], t["faces"], case["voxel"], t["normals"], t["colors"], contraction)   # noqa: E731
    return {"incidences_in_one_cell": 3 * (incidences // 3), "vertices": int(t["verts"].shape[0]), "faces": int(t["faces"].shape[0]),
            "whole_call_quadric_ms": median_ms(lambda: call("quadric"), reps), "whole_call_average_ms": median_ms(lambda: call("average"), reps)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    tsdf, color = fused_scene(dev)
    mesh = marching_cubes(tsdf, 0.0, color, np.array([-1.28, -1.28, 0.0], dtype=np.float32), 0.01)
    out = {"device": torch.cuda.get_device_name(0), "scene": "fused_scene_256", "reps": args.reps,
           "vertices": int(mesh[0].shape[0]), "faces": int(mesh[1].shape[0]), "sample_density_per_m2": DENSITY,
           "timing": "[median, min, max] ms: HIP events around each call (or stage) after 3 warm-up calls",
           "cells": [measure(mesh, voxel, args.reps) for voxel in CELLS], "long_run": long_run(dev, args.reps)}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

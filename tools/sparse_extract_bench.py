"""Device time and memory of the mesh extraction straight from the sparse TSDF volume's pool (csrc/sparse_extract.hip,
``SparseTSDFVolume.mesh_tensors``) against the dense path it replaces -- ``dense()`` and ``marching_cubes`` of its result, unchanged code
-- in the same run, on the scene and lattice of tools/sparse_fuse_bench.py: the three fusing frames of ``fused_scene_256`` (1 cm voxels)
plus one flush of 1, 8 or 32 wavy-wall frames of 256x320.

Per case, HIP events around each call after three warm-up calls, [median, min, max] ms over ``--reps`` calls (Python bindings and their
allocations included, as a caller sees them):
  sparse     neighbour table (device sort + kernel), count, scan + the one host read, emit, and the whole ``mesh_tensors()`` with the
             table cached (the steady case) and rebuilt (the first call after a flush)
  dense      ``dense()``, ``marching_cubes`` on its result, and the two in one call
and, once: the peak extra device memory of one call of either path (torch's allocator statistics), bricks, V and F of both meshes.  (The
dense box here is the allocated bricks' bounding box without margin, so its mesh lacks the triangles that cross the box's faces: V and F
of the two paths need not be equal in this tool; tests/test_sparse_extract_gpu.py compares them where they must be.)
Prints one JSON line; ``--out PATH`` also writes it there.

For the kernels' own durations run one case under the profiler, on its own,
``rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/sparse_extract_bench.py --only 8``, then
``python tools/sparse_extract_bench.py --summarise-trace DIR --only 8 --out profiles/sparse_extract_kernel_trace.json``.

    python tools/sparse_extract_bench.py [--reps 20] [--max-bricks 65536] [--only N] [--out profiles/sparse_extract_bench.json]
"""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
for path in (os.path.join(ROOT, "deep-video-mvs_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, path)

TRACED = ("sparse_neighbours_kernel", "sparse_extract_count_kernel", "sparse_extract_scan_kernel", "sparse_extract_vertices_kernel",
          "sparse_extract_faces_kernel", "sparse_gather_kernel", "mc_count_kernel", "mc_scan_kernel", "mc_vertices_kernel", "mc_faces_kernel")


def summary(values):
    return [round(float(np.median(values)), 4), round(float(np.min(values)), 4), round(float(np.max(values)), 4)]


def event_ms(fn, reps):
    for _ in range(3):
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
    return summary(times)


def peak_extra_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    result = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del result
    return int(peak)


def summarise_trace(folder, only, out):
    """Kernel durations of one traced run: microseconds [median, min, max, dispatches] per kernel of either path, the device sort's together."""
    rows = []
    for name in glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True):
        with open(name, newline="") as f:
            rows += list(csv.DictReader(f))
    kernels = {}
    for row in rows:
        name = row["Kernel_Name"]
        label = next((t for t in TRACED if t in name), "device sort kernels (all)" if "rocprim" in name and "sort" in name else None)
        if label is not None:
            kernels.setdefault(label, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    result = {"what": "kernel durations of tools/sparse_extract_bench.py, one case under rocprofv3 --kernel-trace in a run of its own (tracing slows "
                      "the host, so these are device durations only); the device sort's kernels also serve the flushes of the set-up",
              "command": f"rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/sparse_extract_bench.py --only {only}",
              "n_frames": only, "unit": "microseconds: [median, min, max, dispatches]",
              "kernels": {k: summary(v) + [len(v)] for k, v in sorted(kernels.items())}}
    print(json.dumps(result))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--max-bricks", type=int, default=65536)
    ap.add_argument("--only", type=int, default=None, help="one flush size instead of 1, 8 and 32 (for a kernel trace of the tool)")
    ap.add_argument("--summarise-trace", default=None, metavar="DIR", help="summarise rocprofv3's kernel trace under DIR instead of measuring")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.summarise_trace:
        return summarise_trace(args.summarise_trace, args.only, args.out)
    from dvmvs.hip import sparse as hip_sparse
    from dvmvs.hip.volume import marching_cubes
    from sparse_fuse_bench import ORIGIN, VOXEL, fused_sparse
    from tsdf_fuse_bench import frames
    from tsdf_raycast_bench import H, W
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "scene": "fused_scene_256 + one flush of n_frames wavy-wall frames",
           "voxel_size": VOXEL, "origin": list(ORIGIN), "image": [H, W], "max_bricks": args.max_bricks,
           "timing": "HIP events around each call, Python bindings and allocations included: [median, min, max] ms", "cases": []}
    for n in ((1, 8, 32) if args.only is None else (args.only,)):
        depth, rgb, _, Ks, Ps = frames(n, dev)
        volume = fused_sparse(dev, args.max_bricks)
        volume.integrate_frames(rgb, depth, Ks, Ps)
        state = volume._state
        bricks = volume.n_bricks
        row = {"n_frames": n, "bricks": bricks, "allocated_voxel_bytes": bricks * 512 * 12, "overflow": volume.overflow}
        neighbour = volume.neighbours()
        counts = hip_sparse.sparse_extract_count(state, neighbour)
        offsets, device_summary = hip_sparse.sparse_extract_scan(state, counts)
        _, _, _, V, F = (int(x) for x in device_summary.cpu())

        def scan_and_read():
            return [int(x) for x in hip_sparse.sparse_extract_scan(state, counts)[1].cpu()]

        def rebuilt():
            volume._neighbour = None
            return volume.mesh_tensors()

        def dense_path():
            made = volume.dense()
            return marching_cubes(made._tsdf, 0.0, made._color, made._vol_origin, made._voxel_size)

        row["sparse"] = {
            "neighbours_ms": event_ms(lambda: hip_sparse.sparse_neighbours(state), args.reps),
            "count_ms": event_ms(lambda: hip_sparse.sparse_extract_count(state, neighbour, counts), args.reps),
            "scan_and_host_read_ms": event_ms(scan_and_read, args.reps),
            "emit_ms": event_ms(lambda: hip_sparse.sparse_extract_emit(state, neighbour, offsets, bricks, V, F, volume._origin, volume._voxel_size,
                                                                      colour=False), args.reps),
            "emit_with_colour_ms": event_ms(lambda: hip_sparse.sparse_extract_emit(state, neighbour, offsets, bricks, V, F, volume._origin,
                                                                                  volume._voxel_size, colour=True), args.reps),
            "mesh_tensors_ms": event_ms(volume.mesh_tensors, args.reps),
            "mesh_tensors_table_rebuilt_ms": event_ms(rebuilt, args.reps),
            "vertices": V, "faces": F,
            "neighbour_table_bytes": int(neighbour.numel() * 4), "emit_workspace_bytes": bricks * 729 * 4,
        }
        made = volume.dense()
        dense_mesh = marching_cubes(made._tsdf, 0.0, made._color, made._vol_origin, made._voxel_size)
        row["dense"] = {
            "dims": [int(d) for d in made._tsdf.shape], "volume_bytes": int(made._tsdf.numel()) * 12,
            "dense_call_ms": event_ms(volume.dense, args.reps),
            "marching_cubes_ms": event_ms(lambda: marching_cubes(made._tsdf, 0.0, made._color, made._vol_origin, made._voxel_size), args.reps),
            "dense_plus_marching_cubes_ms": event_ms(dense_path, args.reps),
            "vertices": int(dense_mesh[0].shape[0]), "faces": int(dense_mesh[1].shape[0]),
        }
        del made, dense_mesh
        volume._neighbour = None
        row["sparse"]["peak_extra_bytes_table_rebuilt"] = peak_extra_bytes(volume.mesh_tensors)
        row["sparse"]["peak_extra_bytes_table_cached"] = peak_extra_bytes(volume.mesh_tensors)
        row["dense"]["peak_extra_bytes"] = peak_extra_bytes(dense_path)
        row["sparse_over_dense_time"] = round(row["sparse"]["mesh_tensors_ms"][0] / row["dense"]["dense_plus_marching_cubes_ms"][0], 3)
        row["sparse_rebuilt_over_dense_time"] = round(row["sparse"]["mesh_tensors_table_rebuilt_ms"][0] / row["dense"]["dense_plus_marching_cubes_ms"][0], 3)
        row["sparse_over_dense_peak_bytes"] = round(row["sparse"]["peak_extra_bytes_table_rebuilt"] / max(row["dense"]["peak_extra_bytes"], 1), 4)
        out["cases"].append(row)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

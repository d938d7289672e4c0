"""Device time and memory of ray-casting the sparse TSDF volume straight from its pool (csrc/sparse_raycast.hip,
``SparseTSDFVolume.render``) against the way the same image was made before -- ``dense()`` + ``tsdf_raycast_mask`` + ``TSDFVolume.render``,
unchanged code -- in the same run, on the scene and lattice of tools/sparse_extract_bench.py: the three fusing frames of
``fused_scene_256`` (1 cm voxels) plus one flush of ``--frames`` wavy-wall frames, seen from the views of tools/tsdf_raycast_bench.py at
256x320.

HIP events around each call after three warm-up calls, [median, min, max] ms over ``--reps`` calls (Python bindings and their allocations
included, as a caller sees them):
  sparse     ``render`` of 1 and 16 views with index, flags, neighbour table and the host read cached (the steady case); the first
             ``render`` after a flush (everything rebuilt, one host read); index, flags, neighbour table and the host read on their own
  dense      ``dense()`` + mask + ``render`` of 1 and 16 views (how the image of a growing volume was made before), and the warm
             ``TSDFVolume.render`` alone on a dense copy that already exists (where the sparse gather is expected to lose)
and, once: the peak extra device memory of one call of either path (torch's allocator statistics; for the first render with the
tables of the last state dropped before the baseline is read, so they count: the sparse path KEEPS them until the next flush, the dense
path keeps nothing between calls), and that the images are equal.
Prints one JSON line; ``--out PATH`` also writes it there.

For the kernels' own durations run the tool under the profiler, on its own,
``rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/sparse_raycast_bench.py --reps 5``, then
``python tools/sparse_raycast_bench.py --summarise-trace DIR --out profiles/sparse_raycast_kernel_trace.json``.

    python tools/sparse_raycast_bench.py [--reps 20] [--frames 8] [--max-bricks 65536] [--out profiles/sparse_raycast_bench.json]
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

TRACED = ("sparse_raycast_clear_kernel", "sparse_raycast_index_kernel", "sparse_raycast_flags_kernel", "sparse_raycast_kernel",
          "sparse_neighbours_kernel", "sparse_gather_kernel", "tsdf_raycast_mask_kernel", "tsdf_raycast_kernel")


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


def peak_extra_bytes(fn, prepare=None):
    """Peak device memory of one call above what was allocated when it began; ``prepare`` runs first (to drop what the call rebuilds)."""
    if prepare is not None:
        prepare()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    result = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del result
    return int(peak)


def summarise_trace(folder, out):
    """Kernel durations of one traced run: microseconds [median, min, max, dispatches] per kernel of either path."""
    rows = []
    for name in glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True):
        with open(name, newline="") as f:
            rows += list(csv.DictReader(f))
    kernels = {}
    for row in rows:
        label = next((t for t in TRACED if t in row["Kernel_Name"]), None)
        if label is not None:
            kernels.setdefault(label, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    result = {"what": "kernel durations of tools/sparse_raycast_bench.py under rocprofv3 --kernel-trace in a run of its own (tracing slows the "
                      "host, so these are device durations only); the ray-cast kernels' dispatches mix launches of 1 and 16 views",
              "command": "rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/sparse_raycast_bench.py --reps 5",
              "unit": "microseconds: [median, min, max, dispatches]", "kernels": {k: summary(v) + [len(v)] for k, v in sorted(kernels.items())}}
    print(json.dumps(result))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


def lookup_designs(volume, Kt, poses, H, W, reps):
    """The two key -> slot designs through the SAME kernel (a wave-uniform pointer test chooses per launch), from the tuning library (``make -C deep-video-mvs_amd/csrc tuning``): the
    render index (one probe sequence of an open-addressing table) against the fallback, ``se_find``'s binary search of 32 dependent loads
    over the sorted keys.  Raw C entries, no Python checks on either side; None when the tuning library was not built."""
    import ctypes
    from dvmvs.hip import _capi
    from dvmvs.hip import sparse as hip_sparse
    path = os.path.join(os.path.dirname(_capi.LIB_PATH), "libdvmvs_hip_tuning.so")
    if not os.path.exists(path):
        return None
    lib = ctypes.CDLL(path)
    state = volume._state
    dev = state.device
    status, extent = volume._render_state()
    first, count, low = volume._box("render", None, extent)
    origin = low.astype(np.float32)
    neighbour = volume.neighbours()
    index, flags = volume._render_tables
    slots = torch.arange(state.max_bricks, dtype=torch.int64, device=dev)
    keys = torch.where(slots < state.status[hip_sparse.STATUS_BRICKS], state.pool_key, torch.full_like(state.pool_key, hip_sparse.EMPTY_KEY))
    ordered, order = torch.sort(keys)
    ptr, f, i, ll = (lambda t: ctypes.c_void_p(t.data_ptr())), ctypes.c_float, ctypes.c_int, ctypes.c_longlong
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    results = {}
    images = {}
    for design in ("hash_index", "binary_search"):
        for n in (1, 16):
            Ks = Kt.reshape(1, 3, 3).repeat(n, 1, 1).contiguous()
            depth = torch.empty((n, H, W), dtype=torch.float32, device=dev)
            normal = torch.empty((n, H, W, 3), dtype=torch.float32, device=dev)
            rgb = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
            head = [ptr(state.tsdf), ptr(state.weight), ptr(state.color), ptr(state.status), ll(state.max_bricks), ptr(index), ll(index.shape[0]),
                    ptr(neighbour), ptr(flags)]
            tail = [i(int(first[0])), i(int(first[1])), i(int(first[2])), i(int(count[0])), i(int(count[1])), i(int(count[2])), f(origin[0]),
                    f(origin[1]), f(origin[2]), f(volume.voxel_size), i(1), ptr(Ks), ptr(poses[n]), i(n), i(H), i(W), f(0.0), f(float("inf")),
                    f(1.0), ptr(depth), ptr(normal), ptr(rgb), stream]
            if design == "hash_index":
                def call(head=head, tail=tail):
                    assert lib.dvmvs_sparse_raycast_fwd(*head, *tail) == 0
            else:
                def call(head=head, tail=tail):
                    assert lib.dvmvs_sparse_raycast_fwd_search(*head, ptr(ordered), ptr(order), *tail) == 0
            results[f"{design}_{n}_view{'s' if n > 1 else ''}_ms"] = event_ms(call, reps)
            images[design, n] = (depth, normal, rgb)
    results["images_equal"] = all(torch.equal(a, b) for n in (1, 16) for a, b in zip(images["hash_index", n], images["binary_search", n]))
    results["what"] = "the ray-cast entry of the tuning library called directly (no Python checks, outputs allocated once), skip_empty on"
    return results


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=8, help="wavy-wall frames in the one flush behind the three fusing frames")
    ap.add_argument("--max-bricks", type=int, default=65536)
    ap.add_argument("--summarise-trace", default=None, metavar="DIR", help="summarise rocprofv3's kernel trace under DIR instead of measuring")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.summarise_trace:
        return summarise_trace(args.summarise_trace, args.out)
    from dvmvs.hip import sparse as hip_sparse
    from sparse_fuse_bench import ORIGIN, VOXEL, fused_sparse
    from tsdf_fuse_bench import frames
    from tsdf_raycast_bench import H, K, W, views
    dev = torch.device("cuda:0")
    depth, rgb, _, Ks, Ps = frames(args.frames, dev)
    volume = fused_sparse(dev, args.max_bricks)
    volume.integrate_frames(rgb, depth, Ks, Ps)
    state = volume._state
    bricks = volume.n_bricks
    Kt = torch.from_numpy(K).to(dev)
    poses = {n: torch.from_numpy(np.stack(views(n))).to(dev) for n in (1, 16)}
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "scene": f"fused_scene_256 + one flush of {args.frames} wavy-wall frames",
           "voxel_size": VOXEL, "origin": list(ORIGIN), "image": [H, W], "max_bricks": args.max_bricks, "bricks": bricks,
           "allocated_voxel_bytes": bricks * 512 * 12, "overflow": volume.overflow, "step_voxels": 1.0,
           "timing": "HIP events around each call, Python bindings and allocations included: [median, min, max] ms"}

    def drop():
        volume._neighbour = volume._render_tables = volume._render_read = None

    def first_render():
        drop()
        return volume.render(Kt, poses[1], H, W)

    def host_read():
        volume._render_read = None
        return volume._render_state()

    def dense_path(n):
        return volume.dense().render(Kt, poses[n], H, W)

    made = volume.dense()
    out["box_dims"] = [int(d) for d in made._tsdf.shape]
    out["dense_volume_bytes"] = int(made._tsdf.numel()) * 12
    equal, hits = {}, {}
    for n in (1, 16):
        got, want = volume.render(Kt, poses[n], H, W), made.render(Kt, poses[n], H, W)
        equal[n] = all(torch.equal(a, b) for a, b in zip(got, want))
        hits[n] = round(float((want[0] != 0).float().mean()), 4)
    out["images_equal"], out["hit_share"] = equal, hits
    neighbour = volume.neighbours()
    index, flags = volume._render_tables
    out["flagged_bricks"] = int(flags[:bricks].sum())
    out["sparse"] = {
        "render_1_view_ms": event_ms(lambda: volume.render(Kt, poses[1], H, W), args.reps),
        "render_16_views_ms": event_ms(lambda: volume.render(Kt, poses[16], H, W), args.reps),
        "render_1_view_no_skipping_ms": event_ms(lambda: volume.render(Kt, poses[1], H, W, skip_empty=False), args.reps),
        "render_1_view_depth_only_ms": event_ms(lambda: volume.render(Kt, poses[1], H, W, normals=False, colour=False), args.reps),
        "first_render_after_a_flush_ms": event_ms(first_render, args.reps),
        "index_ms": event_ms(lambda: hip_sparse.sparse_raycast_index(state), args.reps),
        "flags_ms": event_ms(lambda: hip_sparse.sparse_raycast_flags(state, neighbour, index), args.reps),
        "neighbours_ms": event_ms(lambda: hip_sparse.sparse_neighbours(state), args.reps),
        "host_read_ms": event_ms(host_read, args.reps),
        "index_bytes": int(index.numel() * 8), "flags_bytes": int(flags.numel()), "neighbour_table_bytes": int(neighbour.numel() * 4),
    }
    out["dense"] = {
        "dense_mask_render_1_view_ms": event_ms(lambda: dense_path(1), args.reps),
        "dense_mask_render_16_views_ms": event_ms(lambda: dense_path(16), args.reps),
        "dense_call_ms": event_ms(volume.dense, args.reps),
        "warm_render_1_view_ms": event_ms(lambda: made.render(Kt, poses[1], H, W), args.reps),
        "warm_render_16_views_ms": event_ms(lambda: made.render(Kt, poses[16], H, W), args.reps),
        "warm_render_1_view_no_skipping_ms": event_ms(lambda: made.render(Kt, poses[1], H, W, skip_empty=False), args.reps),
    }
    del made
    # (the tables of the last state are dropped BEFORE the baseline is read: a first render allocates them anew and keeps them)
    out["sparse"]["peak_extra_bytes_first_render"] = peak_extra_bytes(lambda: volume.render(Kt, poses[1], H, W), prepare=drop)
    out["sparse"]["tables_kept_bytes"] = out["sparse"]["index_bytes"] + out["sparse"]["flags_bytes"] + out["sparse"]["neighbour_table_bytes"]
    out["sparse"]["peak_extra_bytes_warm"] = peak_extra_bytes(lambda: volume.render(Kt, poses[1], H, W))
    out["dense"]["peak_extra_bytes"] = peak_extra_bytes(lambda: dense_path(1))
    s, d = out["sparse"], out["dense"]
    out["sparse_over_dense_path_time_1_view"] = round(s["render_1_view_ms"][0] / d["dense_mask_render_1_view_ms"][0], 3)
    out["sparse_over_dense_path_time_16_views"] = round(s["render_16_views_ms"][0] / d["dense_mask_render_16_views_ms"][0], 3)
    out["sparse_first_over_dense_path_time_1_view"] = round(s["first_render_after_a_flush_ms"][0] / d["dense_mask_render_1_view_ms"][0], 3)
    out["sparse_over_warm_dense_render_1_view"] = round(s["render_1_view_ms"][0] / d["warm_render_1_view_ms"][0], 3)
    out["sparse_over_warm_dense_render_16_views"] = round(s["render_16_views_ms"][0] / d["warm_render_16_views_ms"][0], 3)
    out["sparse_over_dense_peak_bytes"] = round(s["peak_extra_bytes_first_render"] / max(d["peak_extra_bytes"], 1), 4)
    out["not_measured"] = ["a real scene through python -m dvmvs.tsdf", "pools near capacity", "long empty boxes (parts far apart, no bounds)"]
    out["lookup_designs"] = lookup_designs(volume, Kt, poses, H, W, args.reps)
    if out["lookup_designs"] is None:
        out["not_measured"].append("the binary-search lookup (se_find over the sorted keys) in place of the hash index: it lives in the tuning "
                                   "library only (make -C deep-video-mvs_amd/csrc tuning), which was not built")
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

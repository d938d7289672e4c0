"""Device time and memory of the sparse TSDF volume (csrc/sparse_volume.hip, ``dvmvs.tsdf.SparseTSDFVolume``) against the dense batched
fusion (csrc/tsdf_fuse.hip, ``TSDFVolume.integrate_frames``) in the same run, on the ``fused_scene_256`` scene of tools/tsdf_fuse_bench.py:
a 256^3 volume of 1 cm voxels, the three fusing frames first, then flushes of 1, 8 and 32 wavy-wall frames of 256x320.

Per flush size, HIP events around each step after warm-up, [median, min, max] ms over ``--reps`` flushes:
  steady     flushes into a volume that already holds the scene (the running case: nearly every mark finds its brick): mark, sort + assign,
             integrate, and their sum; these are PER-CALL times of the Python bindings (argument checks included), as a caller sees them
  first      ONE flush of the same frames into an empty volume (every brick is inserted and gets a slot): a single measurement each, after a
             warm-up flush into another volume
  dense      ``TSDFVolume.integrate_frames`` of the same frames into the dense 256^3 volume
and, once: bricks allocated, bytes of allocated voxels against the dense volume's bytes, allocated bricks against those that hold a voxel
with tsdf < 1, rejected pixels, and the time of ``dense()`` (wall clock with synchronisation: it contains its host read and the
allocation of the dense arrays).  Prints one JSON line; ``--out PATH`` also writes it there.

The step times contain the enqueue cost of the bindings (a launch takes the host some 10 us, the sort several launches), so a short step
may be bounded by the host, not the device.  For the kernels' own durations run one flush size under the profiler,
``rocprofv3 --kernel-trace -- python tools/sparse_fuse_bench.py --only 8``: per size the mark kernel is dispatched for the three scene
frames, three warm-up flushes, ``--reps`` steady flushes, TWO flushes into empty volumes (every brick inserted) and the three scene
frames once more, in that order (profiles/sparse_fuse_kernel_trace.json was made that way).

    python tools/sparse_fuse_bench.py [--reps 20] [--max-bricks 65536] [--only N] [--out profiles/sparse_fuse_bench.json]
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

from dvmvs.hip import sparse as hip_sparse  # noqa: E402
from dvmvs.tsdf import SparseTSDFVolume  # noqa: E402
from tsdf_fuse_bench import frames  # noqa: E402
from tsdf_raycast_bench import H, K, W, fused_scene  # noqa: E402

VOXEL = 0.01
ORIGIN = (-1.28, -1.28, 0.0)


def base_frames():
    """The three frames of ``fused_scene``."""
    y, x = np.meshgrid(np.arange(float(H)), np.arange(float(W)), indexing="ij")
    depth = np.stack([(1.2 + 0.2 * np.sin(x / 40 + n) + 0.1 * np.cos(y / 30)).astype(np.float32) for n in range(3)])
    rgb = np.stack([np.stack([x % 256, y % 256, (x + y + 40 * n) % 256], -1).astype(np.uint8) for n in range(3)])
    poses = np.repeat(np.eye(4, dtype=np.float32)[None], 3, axis=0)
    poses[:, 0, 3] = [0.0, 0.05, 0.1]
    return rgb, depth, poses


def fused_sparse(dev, max_bricks):
    volume = SparseTSDFVolume(VOXEL, origin=ORIGIN, max_bricks=max_bricks, device=dev)
    rgb, depth, poses = base_frames()
    for n in range(3):
        volume.integrate(rgb[n], depth[n], K, poses[n])
    return volume


def stages(volume, data, timed=True):
    """One flush of ``data`` into ``volume`` step by step; the three step times in ms (HIP events)."""
    depth, rgb, _, Ks, Ps = data
    n = depth.shape[0]
    state, first = volume._state, volume.frames
    volume.frames += n
    events = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    events[0].record()
    hip_sparse.sparse_mark(state, depth, Ks, Ps, volume._origin, volume._voxel_size, volume._trunc_margin, float("inf"), first)
    events[1].record()
    hip_sparse.sparse_assign(state)
    events[2].record()
    hip_sparse.sparse_integrate(state, depth, Ks, Ps, rgb, None, volume._origin, volume._voxel_size, volume._trunc_margin, [1.0] * n,
                                float("inf"), first)
    events[3].record()
    if not timed:
        return None
    torch.cuda.synchronize()
    return [events[i].elapsed_time(events[i + 1]) for i in range(3)]


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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--max-bricks", type=int, default=65536)
    ap.add_argument("--only", type=int, default=None, help="one flush size instead of 1, 8 and 32 (for a kernel trace of the tool)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    dense = fused_scene(dev)
    dense_bytes = int(dense._tsdf.numel()) * 12
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "scene": "fused_scene_256", "voxel_size": VOXEL, "image": [H, W],
           "max_bricks": args.max_bricks, "dense_dims": [int(d) for d in dense._tsdf.shape], "dense_volume_bytes": dense_bytes,
           "timing": "HIP events around each step of a flush, Python bindings included: [median, min, max] ms", "cases": []}
    for n in ((1, 8, 32) if args.only is None else (args.only,)):
        data = frames(n, dev)
        depth, rgb, _, Ks, Ps = data
        row = {"n_frames": n}
        volume = fused_sparse(dev, args.max_bricks)
        for _ in range(3):
            stages(volume, data, timed=False)
        torch.cuda.synchronize()
        times = np.array([stages(volume, data) for _ in range(args.reps)])
        row["steady"] = {"mark_ms": summary(times[:, 0]), "sort_assign_ms": summary(times[:, 1]), "integrate_ms": summary(times[:, 2]),
                         "flush_ms": summary(times.sum(axis=1))}
        stages(SparseTSDFVolume(VOXEL, origin=ORIGIN, max_bricks=args.max_bricks, device=dev), data, timed=False)     # warm-up
        torch.cuda.synchronize()
        fresh = SparseTSDFVolume(VOXEL, origin=ORIGIN, max_bricks=args.max_bricks, device=dev)
        first = stages(fresh, data)
        row["first"] = {"mark_ms": round(first[0], 4), "sort_assign_ms": round(first[1], 4), "integrate_ms": round(first[2], 4),
                        "flush_ms": round(sum(first), 4), "bricks": fresh.n_bricks}
        row["dense_integrate_frames_ms"] = event_ms(lambda: dense.integrate_frames(rgb, depth, Ks, Ps), args.reps)
        row["sparse_over_dense_steady"] = round(row["steady"]["flush_ms"][0] / row["dense_integrate_frames_ms"][0], 3)
        # what the scene plus this flush's frames occupy
        bricks = volume.n_bricks
        in_band = int((volume.pool()[0][:bricks] < 1).any(dim=1).sum())
        row.update({"bricks": bricks, "bricks_with_tsdf_below_1": in_band, "marked_over_in_band": round(bricks / max(in_band, 1), 3),
                    "allocated_voxel_bytes": bricks * 512 * 12, "allocated_over_dense_bytes": round(bricks * 512 * 12 / dense_bytes, 5),
                    "overflow": volume.overflow, "rejected_pixels": volume.rejected_pixels})
        torch.cuda.synchronize()
        walls = []
        for _ in range(5):
            t0 = time.perf_counter()
            made = volume.dense()
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        row["dense_call_wall_ms"] = summary(walls)
        row["dense_call_dims"] = [int(d) for d in made._tsdf.shape]
        out["cases"].append(row)
    state = fused_sparse(dev, args.max_bricks)._state
    out["pool_bytes_reserved"] = int(sum(t.numel() * t.element_size() for t in (state.tsdf, state.weight, state.color)))
    out["table_and_scratch_bytes"] = int(sum(t.numel() * t.element_size() for t in (state.table_keys, state.table_birth, state.fresh, state.sorted,
                                                                                    state.sort_index, state.pool_key, state.pool_birth)))
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

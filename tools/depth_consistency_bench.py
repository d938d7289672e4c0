"""Device time of the depth-map consistency filter (csrc/depth_consistency.hip) at 256x320 on the analytic scene of
tests/consistency_reference.py (a plane and a sphere, rendered exactly), seen from N cameras on a slow arc, four sources per frame
(``nearest_sources``).

op       one ``ops.depth_consistency`` call (matrices launch + pixel launch; depth and count out), and the pixel launch alone with the
         matrices given: HIP events around each call after warm-up, [median, min, max] ms over ``--reps`` calls.
torch    the same float32 procedure as element-wise torch operations and gathers on the device, one pass per slot over all frames (eager
         torch rounds every operation on its own, so depth and count must be EQUAL to the op's, which is checked).  Timed the same way,
         ALTERNATING with the op in the same process: op, torch, op, torch, ...
bytes    the algorithmic bytes N H W (4 read + 4 written + 1 count) over the pixel launch's median time, as a share of the HBM bandwidth
         (6.29 TB/s measured with a float4 copy; 8 TB/s on paper).  The gathered taps (16 bytes per pixel and non-skipped slot) are
         listed beside it; they are served by L2 and are not part of the share.
flush    a ``LiveFusion`` flush of 8 pending frames into a 200x150x75 volume of 2 cm voxels, with and without ``min_consistent_views=2``,
         alternated likewise.
Prints one JSON line; ``--out PATH`` also writes it there.

    python tools/depth_consistency_bench.py [--reps 30] [--out profiles/depth_consistency_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
for path in (os.path.join(ROOT, "deep-video-mvs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, path)

import consistency_reference as cr  # noqa: E402
from dvmvs.consistency import nearest_sources  # noqa: E402
from dvmvs.hip import ops  # noqa: E402
from dvmvs.tsdf import LiveFusion  # noqa: E402

H, W, FOCAL = 256, 320, 300.0
HBM_MEASURED, HBM_PAPER = 6.29e12, 8.0e12
BOUNDS = np.array([[-2.0, 2.0], [-1.5, 1.5], [1.0, 2.5]])


def scene(n, dev):
    """n views on an arc: 1.5 cm and 2.5 mrad from one to the next, so that four neighbours on either side still overlap."""
    K = cr.intrinsics(H, W, FOCAL)
    poses = []
    for i in range(n):
        a = 0.0025 * (i - (n - 1) / 2)
        pose = np.eye(4, dtype=np.float32)
        pose[:3, :3] = [[np.cos(a), 0, -np.sin(a)], [0, 1, 0], [np.sin(a), 0, np.cos(a)]]
        pose[:3, 3] = [0.015 * (i - (n - 1) / 2), 0.004 * (i % 5), 0.003 * (i % 3)]
        poses.append(pose)
    poses = np.stack(poses)
    depths = np.stack([cr.render(K, p, H, W) for p in poses])
    to = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)   # noqa: E731
    return to(depths), to(np.repeat(K[None], n, axis=0)), to(poses), to(nearest_sources(n, 4))


def torch_filter(depths, sources, matrices, pixel_threshold=1.0, relative_threshold=0.01, min_views=2, average=True):
    """Step B of include/dvmvs_hip.h in eager torch, one pass per slot over all frames."""
    N, Hh, Ww = depths.shape
    f32 = torch.float32
    v, u = torch.meshgrid(torch.arange(Hh, device=depths.device, dtype=f32), torch.arange(Ww, device=depths.device, dtype=f32), indexing="ij")
    u, v = u[None], v[None]
    valid = torch.isfinite(depths) & (depths > 0)
    count = torch.zeros_like(depths, dtype=torch.int32)
    total = depths.clone()
    flat = depths.reshape(N, Hh * Ww)
    frames = torch.arange(N, device=depths.device, dtype=torch.int64)
    thr2 = float(np.float32(pixel_threshold) * np.float32(pixel_threshold))
    for j in range(sources.shape[1]):
        s = sources[:, j].long()
        live = (s >= 0) & (s < N) & (s != frames)
        src = flat[s.clamp(0, N - 1)]
        m = matrices[:, j].reshape(N, 24, 1, 1)
        px = depths * ((m[:, 0] * u + m[:, 1] * v) + m[:, 2]) + m[:, 9]
        py = depths * ((m[:, 3] * u + m[:, 4] * v) + m[:, 5]) + m[:, 10]
        pz = depths * ((m[:, 6] * u + m[:, 7] * v) + m[:, 8]) + m[:, 11]
        us, vs = px / pz, py / pz
        inside = valid & live[:, None, None] & (pz > 0) & (us >= 0) & (us <= Ww - 1) & (vs >= 0) & (vs <= Hh - 1)
        us, vs = torch.where(inside, us, torch.zeros_like(us)), torch.where(inside, vs, torch.zeros_like(vs))
        x0, y0 = us.floor().clamp(max=Ww - 2), vs.floor().clamp(max=Hh - 2)
        wx, wy = us - x0, vs - y0
        base = (y0.long() * Ww + x0.long()).reshape(N, -1)
        t00, t01, t10, t11 = (torch.gather(src, 1, base + o).reshape(N, Hh, Ww) for o in (0, 1, Ww, Ww + 1))
        taps = inside
        for t in (t00, t01, t10, t11):
            taps = taps & torch.isfinite(t) & (t > 0)
        top, bot = t00 + wx * (t01 - t00), t10 + wx * (t11 - t10)
        ds = top + wy * (bot - top)
        qx = ds * ((m[:, 12] * us + m[:, 13] * vs) + m[:, 14]) + m[:, 21]
        qy = ds * ((m[:, 15] * us + m[:, 16] * vs) + m[:, 17]) + m[:, 22]
        qz = ds * ((m[:, 18] * us + m[:, 19] * vs) + m[:, 20]) + m[:, 23]
        du, dv = qx / qz - u, qy / qz - v
        ok = taps & (qz > 0) & (du * du + dv * dv < thr2) & ((qz - depths).abs() / depths < relative_threshold)
        count += ok
        total = torch.where(ok, total + qz, total)
    fused = total / (count + 1).to(f32)
    keep = valid & (count >= min_views)
    return torch.where(keep, fused if average else depths, torch.zeros_like(depths)), torch.where(valid, count, 0).to(torch.uint8)


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end)


def alternate(fns, reps):
    """{name: [median, min, max] ms}: the functions take turns, ``reps`` times, after three warm-up rounds."""
    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            times[name].append(timed(fn))
    return {name: [round(float(np.median(t)), 4), round(float(np.min(t)), 4), round(float(np.max(t)), 4)] for name, t in times.items()}


def filter_case(n, dev, reps):
    depths, K, poses, sources = scene(n, dev)
    matrices = ops.consistency_matrices(K, poses, sources)
    depth, count, _ = ops.depth_consistency(depths, K, poses, sources, matrices=matrices)
    want_depth, want_count = torch_filter(depths, sources, matrices)
    equal = bool(torch.equal(depth.view(torch.int32), want_depth.view(torch.int32)) and torch.equal(count, want_count))
    times = alternate({"op_ms": lambda: ops.depth_consistency(depths, K, poses, sources),
                       "pixel_launch_ms": lambda: ops.depth_consistency(depths, K, poses, sources, matrices=matrices),
                       "torch_ms": lambda: torch_filter(depths, sources, matrices)}, reps)
    slots = int(((sources >= 0) & (sources < n)).sum())
    algorithmic = n * H * W * 9
    seconds = times["pixel_launch_ms"][0] * 1e-3
    case = {"N": n, "S": int(sources.shape[1]), "kept_share_of_valid": round(float((depth > 0).sum()) / float((depths > 0).sum()), 4),
            "torch_equal_bitwise": equal, **times, "torch_over_op": round(times["torch_ms"][0] / times["op_ms"][0], 1),
            "algorithmic_bytes": algorithmic, "gathered_tap_bytes": slots * H * W * 16,
            "share_of_hbm_measured_6.29TBs": round(algorithmic / seconds / HBM_MEASURED, 4),
            "share_of_hbm_paper_8TBs": round(algorithmic / seconds / HBM_PAPER, 4)}
    return case, equal


def flush_case(dev, reps):
    depths, K, poses, _ = scene(8, dev)
    rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
    lives = {}
    for name, views in (("flush_ms", 0), ("flush_filtered_ms", 2)):
        live = LiveFusion(BOUNDS.copy(), voxel_size=0.02, max_depth=5.0, batch=9, device=dev, min_consistent_views=views)
        for i in range(8):
            live.add(depths[i], rgb, K[i].cpu().numpy(), poses[i].cpu().numpy())
        lives[name] = live

    def flush(live):
        live._pending, live._weights = 8, [1.0] * 8        # the rings still hold the eight frames: fuse them again
        live.flush()

    times = alternate({name: (lambda live=live: flush(live)) for name, live in lives.items()}, reps)
    return {"frames": 8, "volume": [int(d) for d in lives["flush_ms"].volume.vol_dim], "voxel_size": 0.02, **times}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this benchmark measures on an MI355X; no GPU is visible")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "size": [H, W], "reps": args.reps,
           "timing": "HIP events around each call after warm-up, the candidates alternating in one process: [median, min, max] ms"}
    all_equal = True
    cases = []
    for n in (8, 64):
        case, equal = filter_case(n, dev, args.reps)
        cases.append(case)
        all_equal &= equal
    out["filter"] = cases
    out["live_fusion"] = flush_case(dev, args.reps)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    if not all_equal:
        raise SystemExit("the op and the torch restatement disagree")


if __name__ == "__main__":
    main()

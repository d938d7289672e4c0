"""Device time of the TSDF ray-caster (csrc/tsdf_raycast.hip) on the fused synthetic scene of tools/marching_cubes_bench.py
(256^3 voxels of 1 cm, three frames of a wavy wall), 256x320 views, N = 1 and N = 16.

HIP events around batches of op calls after warm-up, medians over ``--reps`` batches: the brick-mask build, the march with and without
empty-space skipping, each with depth only and with normals and colour.  These are PER-CALL times of ``dvmvs.hip.ops`` (argument checks
and output allocation included), not kernel durations; for those, trace the tool with ``--no-torch`` under ``rocprofv3 --kernel-trace``.  Both marches are checked to give the same bits.  As the yardstick
for "what a user would do without this kernel", the same file records a plain torch dense march at the same step: ``F.grid_sample`` on the
volume, one call per step (tsdf and an observed-flag channel, trilinear), with the same bracket rule (its validity is the interpolated
flag, so next to unobserved voxels it can differ from the kernel; the file records how often).  That march is some 300 steps of about
fifteen small torch launches each: at these sizes it is bound by launch overhead, not by ``grid_sample``'s throughput, and is recorded as
what such a loop costs, not as what the device could do.  Its step count is read back once, outside the timed calls.
Prints one JSON line; ``--out PATH`` also writes it there.

    python tools/tsdf_raycast_bench.py [--reps 20] [--out profiles/tsdf_raycast_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "deep-video-mvs_amd"))

from dvmvs.hip import ops  # noqa: E402
from dvmvs.tsdf import TSDFVolume  # noqa: E402

H, W = 256, 320
K = np.array([[300.0, 0, 159.5], [0, 300.0, 127.5], [0, 0, 1.0]], dtype=np.float32)


def fused_scene(dev):
    """The ``fused_scene_256`` volume of tools/marching_cubes_bench.py."""
    vol = TSDFVolume(np.array([[-1.28, 1.28], [-1.28, 1.28], [0.0, 2.56]]), 0.01, device=dev)
    y, x = np.meshgrid(np.arange(256.0), np.arange(320.0), indexing="ij")
    for n in range(3):
        depth = (1.2 + 0.2 * np.sin(x / 40 + n) + 0.1 * np.cos(y / 30)).astype(np.float32)
        rgb = np.stack([x % 256, y % 256, (x + y + 40 * n) % 256], -1).astype(np.uint8)
        pose = np.eye(4)
        pose[0, 3] = 0.05 * n
        vol.integrate(rgb, depth, K, pose)
    return vol


def views(n):
    """n camera-to-world poses around the fusing cameras: small yaws and shifts, all facing the wall."""
    poses = []
    for i in range(n):
        a = 0.02 * (i - (n - 1) / 2)
        pose = np.eye(4, dtype=np.float32)
        pose[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        pose[:3, 3] = [0.05 + 0.01 * i, 0.005 * i, 0.02 * (i % 3)]
        poses.append(pose)
    return np.stack(poses)


def median_ms(fn, reps, inner):
    """Median over ``reps`` event-timed batches of ``inner`` calls, per call."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(inner):
            fn()
        end.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(end) / inner)
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def torch_dense_march(tsdf, weight, origin, voxel_size, Kt, poses, step, n_steps=None):
    """The same march in plain torch: per step one ``grid_sample`` of (tsdf, observed) at every ray's sample, then the bracket rule.
    Rays start where they enter the box (or at the camera); the loop covers the longest ray (one host read, unless ``n_steps`` is
    given).  Returns (depth, number of steps)."""
    N = poses.shape[0]
    X, Y, Z = tsdf.shape
    vol = torch.stack([tsdf, (weight > 0).float()])[None]                          # [1,2,X,Y,Z]
    v, u = torch.meshgrid(torch.arange(H, device=tsdf.device, dtype=torch.float32), torch.arange(W, device=tsdf.device, dtype=torch.float32),
                          indexing="ij")
    dc = torch.stack([(u - Kt[0, 2]) / Kt[0, 0], (v - Kt[1, 2]) / Kt[1, 1], torch.ones_like(u)], -1)        # [H,W,3]
    dg = torch.einsum("nij,hwj->nhwi", poses[:, :3, :3], dc) / voxel_size
    og = ((poses[:, :3, 3] - origin) / voxel_size)[:, None, None, :]
    hi = torch.tensor([X - 1, Y - 1, Z - 1], device=tsdf.device, dtype=torch.float32)
    ta, tb = (0 - og) / dg, (hi - og) / dg
    z0 = torch.minimum(ta, tb).amax(-1).clamp_min(0.0)
    z1 = torch.maximum(ta, tb).amin(-1)
    dz = step / dg.norm(dim=-1)
    if n_steps is None:
        n_steps = int(torch.floor(((z1 - z0) / dz).clamp_min(-1.0).max()).item()) + 1
    depth = torch.zeros((N, H, W), device=tsdf.device)
    prev_f = torch.zeros_like(depth)
    prev_ok = torch.zeros_like(depth, dtype=torch.bool)
    for k in range(n_steps):
        z = z0 + k * dz
        g = og + z[..., None] * dg
        grid = (2 * g / hi - 1).flip(-1)[None]                                     # grid_sample's x is the last (z) axis
        s = F.grid_sample(vol, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0]      # [2,N,H,W]
        f, ok = s[0], (s[1] > 0.9999) & (z <= z1)          # (the interpolated flag: 1 up to rounding when all corners are observed)
        new = (depth == 0) & ok & prev_ok & (prev_f > 0) & (f <= 0)
        depth = torch.where(new, z - dz + dz * prev_f / (prev_f - f), depth)
        prev_f, prev_ok = f, ok
    return depth, n_steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", type=float, default=1.0)
    ap.add_argument("--no-torch", action="store_true", help="leave the torch yardstick out (for a kernel trace of the tool)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    vol = fused_scene(dev)
    tsdf, weight, color = vol._tsdf, vol._weight, vol._color
    origin, voxel = [float(o) for o in vol._vol_origin], vol._voxel_size
    X, Y, Z = tsdf.shape
    mask = ops.tsdf_raycast_mask(tsdf, weight)
    t_mask = median_ms(lambda: ops.tsdf_raycast_mask(tsdf, weight, out=mask), args.reps, 10)
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "scene": "fused_scene_256", "dims": [X, Y, Z], "image": [H, W],
           "step_voxels": args.step, "timing": "HIP events around batches of op calls, per call (checks and allocation included): [median, min, max] ms",
           "bricks": int(mask.numel()), "bricks_flagged": int(mask.sum()), "mask_build_ms": [round(t, 4) for t in t_mask], "cases": []}
    Kt = torch.from_numpy(K).to(dev)
    for n in (1, 16):
        poses = torch.from_numpy(views(n)).to(dev)
        Ks = Kt[None].expand(n, 3, 3).contiguous()

        def run(m, extras):
            return ops.tsdf_raycast(tsdf, weight, color, origin, voxel, Ks, poses, H, W, step=args.step, mask=m, normals=extras, colour=extras)

        dense, skipped = run(None, True), run(mask, True)
        same = all(torch.equal(a, b) for a, b in zip(dense, skipped))
        row = {"n_views": n, "hit_share": round(float((dense[0] > 0).float().mean()), 4), "skip_equals_dense_bitwise": same}
        inner = 10 if n == 1 else 3
        for label, m in (("skip", mask), ("dense", None)):
            for tag, extras in (("depth_only", False), ("depth_normals_colour", True)):
                row[f"{label}_{tag}_ms"] = [round(t, 4) for t in median_ms(lambda: run(m, extras), args.reps, inner)]
        if args.no_torch:
            out["cases"].append(row)
            continue
        # the torch yardstick: as many steps as the longest ray of these views needs
        origin_t = torch.tensor(origin, device=dev)
        ref, n_steps = torch_dense_march(tsdf, weight, origin_t, voxel, Kt, poses, args.step)
        both = (ref > 0) & (dense[0] > 0)
        row["torch_grid_sample_steps"] = n_steps
        row["torch_grid_sample_ms"] = [round(t, 3) for t in median_ms(
            lambda: torch_dense_march(tsdf, weight, origin_t, voxel, Kt, poses, args.step, n_steps), args.reps, 1)]
        row["torch_grid_sample_note"] = "launch-bound: about 15 small launches per step"
        row["torch_hit_share"] = round(float((ref > 0).float().mean()), 4)
        # (the yardstick interpolates an observed-flag, so next to unobserved voxels it may bracket elsewhere than the kernel does)
        diff = (ref - dense[0]).abs()[both]
        row["torch_vs_kernel_median_abs_depth_m"] = float(diff.median()) if bool(both.any()) else None
        row["torch_vs_kernel_share_of_hits_beyond_1mm"] = round(float((diff > 1e-3).float().mean()), 6) if bool(both.any()) else None
        out["cases"].append(row)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

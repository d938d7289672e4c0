"""Device time of the marching-cubes launches (csrc/marching_cubes.hip) on a 256^3 sphere SDF and on a fused synthetic scene.

HIP events around each call after warm-up; per pass: count (passes 1 + 2), the one host read of V / F, emit (passes 3 + 4).
Reports voxels/s and GB/s of volume bytes read (the volume is read once per streaming pass: count, vertices, faces).
Prints one JSON line; ``--out PATH`` also writes it there.

    python tools/marching_cubes_bench.py [--reps 20] [--out profiles/marching_cubes_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
for p in (os.path.join(ROOT, "deep-video-mvs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from dvmvs.hip import _capi  # noqa: E402
from dvmvs.tsdf import TSDFVolume, marching_cubes  # noqa: E402


def sphere_volume(n, r, dev):
    g = torch.arange(n, device=dev, dtype=torch.float32) - (n - 1) / 2
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    return (torch.sqrt(x * x + y * y + z * z) - r).contiguous()


def fused_scene(dev):
    """256^3 voxels of 1 cm; three frames of a wavy wall seen from slightly different positions."""
    vol = TSDFVolume(np.array([[-1.28, 1.28], [-1.28, 1.28], [0.0, 2.56]]), 0.01, device=dev)
    K = np.array([[300.0, 0, 159.5], [0, 300.0, 127.5], [0, 0, 1.0]])
    y, x = np.meshgrid(np.arange(256.0), np.arange(320.0), indexing="ij")
    for n in range(3):
        depth = (1.2 + 0.2 * np.sin(x / 40 + n) + 0.1 * np.cos(y / 30)).astype(np.float32)
        rgb = np.stack([x % 256, y % 256, (x + y + 40 * n) % 256], -1).astype(np.uint8)
        pose = np.eye(4)
        pose[0, 3] = 0.05 * n
        vol.integrate(rgb, depth, K, pose)
    return vol._tsdf, vol._color


def time_case(name, vol, color, reps):
    dev = vol.device
    lib = _capi.lib()
    X, Y, Z = vol.shape
    nbytes = lib.dvmvs_marching_cubes_workspace_bytes(X, Y, Z)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for _ in range(3):
        verts, faces, normals, colors = marching_cubes(vol, 0.0, color)
    V, F = len(verts), len(faces)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    t_count, t_emit = [], []
    for _ in range(reps):
        ev[0].record()
        _capi.check(lib.dvmvs_marching_cubes_count(vol.data_ptr(), X, Y, Z, 0.0, ws.data_ptr(), nbytes, counts.data_ptr(), stream), "count")
        ev[1].record()
        _capi.check(lib.dvmvs_marching_cubes_emit(vol.data_ptr(), None if color is None else color.data_ptr(), X, Y, Z, 0.0, 0.0, 0.0, 0.0,
                                                  1.0, ws.data_ptr(), verts.data_ptr(), normals.data_ptr(),
                                                  None if colors is None else colors.data_ptr(), faces.data_ptr(), V, F, stream), "emit")
        ev[2].record()
        torch.cuda.synchronize()
        t_count.append(ev[0].elapsed_time(ev[1]))
        t_emit.append(ev[1].elapsed_time(ev[2]))
    c, e = float(np.median(t_count)), float(np.median(t_emit))
    total = c + e
    # wall time of the Python call, host read of the counts and output allocation included
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        marching_cubes(vol, 0.0, color)
    end.record()
    torch.cuda.synchronize()
    n_vox = X * Y * Z
    return {"case": name, "dims": [X, Y, Z], "vertices": V, "faces": F, "colour": color is not None,
            "count_ms": round(c, 4), "emit_ms": round(e, 4), "device_total_ms": round(total, 4),
            "python_call_ms": round(start.elapsed_time(end) / reps, 4),
            "gvoxels_per_s": round(n_vox / total / 1e6, 2), "volume_gb_per_s_3_passes": round(3 * 4 * n_vox / total / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = [time_case("sphere_256_r100", sphere_volume(256, 100.0, dev), None, args.reps)]
    tsdf, color = fused_scene(dev)
    rows.append(time_case("fused_scene_256", tsdf, color, args.reps))
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "cases": rows}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

"""Device time of the mesh rasteriser (csrc/mesh_raster.hip) on the fused synthetic scene of tools/marching_cubes_bench.py (256^3 voxels of
1 cm, three frames of a wavy wall): its own marching-cubes mesh (some 190 000 faces of a few pixels each) and the same wall as a
coarse mesh of 384 faces of some 400 pixels each, and a closed box of 12 triangles around the cameras (faces that cover much of the image
and cross the camera plane); 256x320 views, N = 1 and N = 16.

ops      ``ops.mesh_raster`` and ``ops.mesh_visibility`` (against the rasteriser's own depth maps): HIP events around batches of calls after
         warm-up, [median, min, max] ms per call over ``--reps`` batches.  PER-CALL times of the ops (argument checks, the world-to-camera
         matrices and the output allocation included), not kernel durations.
sweep    the same call with ``large_box`` (the box size from which a clipped triangle goes to the device work list instead of being
         rasterised by the thread of its face) over a few values, on both meshes: the shipped ``MESH_RASTER_LARGE_BOX`` is chosen from
         this table.  Every value must give the same bits.
eager    the same definition as vectorised eager torch on the device, for the fine mesh (where every box is small enough to enumerate):
         float32 operations in the definition's order, int64 edge functions over every (face, pixel of its box) pair, int64 keys and
         ``scatter_reduce_`` with ``amin``; faces in chunks, views in a loop.  It does not clip (no face of this scene comes near the
         camera plane; checked).  Checked first: depth and face must be EQUAL bit for bit.  Timed the same way.
renderers the median absolute difference, in voxels, between ``render_mesh(volume.mesh_tensors())`` and ``volume.render()`` over the pixels
         both hit: two independent renderers of one surface.  A recorded number.
Prints one JSON line; ``--out PATH`` also writes it there.

    python tools/mesh_raster_bench.py [--reps 20] [--out profiles/mesh_raster_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
for path in (os.path.join(ROOT, "deep-video-mvs_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, path)

from dvmvs.hip import ops  # noqa: E402
from dvmvs.hip.ops import reconstruction  # noqa: E402
from dvmvs.tsdf import render_mesh  # noqa: E402
from tsdf_raycast_bench import H, K, W, fused_scene, median_ms, views  # noqa: E402

NEAR = 0.05
SWEEP = (16, 64, 256, 1024, 4096, 10 ** 9)
I64_MAX = 0x7fffffffffffffff


def coarse_wall(rows=12, cols=16):
    """The wall of frame 0 of the scene as a grid of 2 rows cols triangles, back-projected from its depth function."""
    y, x = np.meshgrid(np.linspace(0.0, H - 1.0, rows + 1), np.linspace(0.0, W - 1.0, cols + 1), indexing="ij")
    z = 1.2 + 0.2 * np.sin(x / 40) + 0.1 * np.cos(y / 30)
    verts = np.stack([(x - K[0, 2]) / K[0, 0] * z, (y - K[1, 2]) / K[1, 1] * z, z], axis=-1).reshape(-1, 3).astype(np.float32)
    index = np.arange((rows + 1) * (cols + 1)).reshape(rows + 1, cols + 1)
    a, b, c, d = index[:-1, :-1].ravel(), index[:-1, 1:].ravel(), index[1:, :-1].ravel(), index[1:, 1:].ravel()
    return verts, np.concatenate([np.stack([a, b, c], axis=1), np.stack([b, d, c], axis=1)]).astype(np.int32)


def box_around(half=1.3, centre=(0.0, 0.0, 1.0)):
    """A closed box of 12 triangles around the cameras: every face covers a large part of every image and crosses the camera plane."""
    c = np.asarray(centre, dtype=np.float32)
    verts = np.array([[x, y, z] for x in (-half, half) for y in (-half, half) for z in (-half, half)], dtype=np.float32) + c
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    faces = [t for a, b, c_, d in quads for t in ((a, b, c_), (a, c_, d))]
    return verts, np.array(faces, dtype=np.int32)


def eager_raster(verts, faces, Kt, w2c, height, width, chunk=1 << 16):
    """The definition in eager torch (module docstring).  Returns (depth, face, largest box side, faces that would need clipping)."""
    dev = verts.device
    N = Kt.shape[0]
    tri = faces.long()
    keys = torch.full((N, height * width), I64_MAX, dtype=torch.int64, device=dev)
    side, behind = 0, 0
    for r in range(N):
        fx, fy, cx, cy = Kt[r, 0, 0], Kt[r, 1, 1], Kt[r, 0, 2], Kt[r, 1, 2]
        M = w2c[r]
        x, y, z = verts[:, 0], verts[:, 1], verts[:, 2]
        cam = torch.stack([((M[i, 0] * x + M[i, 1] * y) + M[i, 2] * z) + M[i, 3] for i in range(3)], dim=1)
        sx = torch.round(256.0 * ((cam[:, 0] / cam[:, 2]) * fx + cx)).long()
        sy = torch.round(256.0 * ((cam[:, 1] / cam[:, 2]) * fy + cy)).long()
        behind += int((cam[:, 2] < NEAR).sum())
        for first in range(0, tri.shape[0], chunk):
            t = tri[first:first + chunk]
            p = [cam[t[:, j]] for j in range(3)]
            e1, e2 = p[1] - p[0], p[2] - p[0]
            nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
            ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
            nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
            na = (nx * p[0][:, 0] + ny * p[0][:, 1]) + nz * p[0][:, 2]
            lo = torch.clamp(torch.minimum(torch.minimum(p[0][:, 2], p[1][:, 2]), p[2][:, 2]), min=NEAR)
            hi = torch.maximum(torch.maximum(p[0][:, 2], p[1][:, 2]), p[2][:, 2])
            X, Y = [sx[t[:, j]] for j in range(3)], [sy[t[:, j]] for j in range(3)]
            area = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
            flip = area < 0
            X[1], X[2] = torch.where(flip, X[2], X[1]), torch.where(flip, X[1], X[2])
            Y[1], Y[2] = torch.where(flip, Y[2], Y[1]), torch.where(flip, Y[1], Y[2])
            u0 = torch.clamp((torch.minimum(torch.minimum(X[0], X[1]), X[2]) + 255) >> 8, min=0)
            u1 = torch.clamp(torch.maximum(torch.maximum(X[0], X[1]), X[2]) >> 8, max=width - 1)
            v0 = torch.clamp((torch.minimum(torch.minimum(Y[0], Y[1]), Y[2]) + 255) >> 8, min=0)
            v1 = torch.clamp(torch.maximum(torch.maximum(Y[0], Y[1]), Y[2]) >> 8, max=height - 1)
            B = int(max((u1 - u0).max(), (v1 - v0).max())) + 1              # a host read per chunk: inside the time, as a user would pay it
            side = max(side, B)
            if B < 1:
                continue
            off = torch.arange(B, device=dev)
            u = u0[:, None, None] + off[None, None, :]
            v = v0[:, None, None] + off[None, :, None]
            covered = (u <= u1[:, None, None]) & (v <= v1[:, None, None]) & (area != 0)[:, None, None]
            for i in range(3):
                j = (i + 1) % 3
                dx, dy = X[j] - X[i], Y[j] - Y[i]
                top_left = (dy < 0) | ((dy == 0) & (dx > 0))
                E = dx[:, None, None] * (256 * v - Y[i][:, None, None]) - dy[:, None, None] * (256 * u - X[i][:, None, None])
                covered &= (E > 0) | ((E == 0) & top_left[:, None, None])
            rx = (u.float() - cx) / fx
            ry = (v.float() - cy) / fy
            den = (nx[:, None, None] * rx + ny[:, None, None] * ry) + nz[:, None, None]
            depth = na[:, None, None] / den
            depth = torch.minimum(torch.maximum(torch.nan_to_num(depth, nan=-1.0), lo[:, None, None]), hi[:, None, None])
            index = torch.arange(first, first + t.shape[0], device=dev)[:, None, None]
            key = (depth.view(torch.int32).long() << 32) | index
            pixel = (v * width + u).clamp(0, height * width - 1)
            keys[r].scatter_reduce_(0, pixel[covered], key.expand_as(pixel)[covered], reduce="amin")
    hit = keys != I64_MAX
    depth = torch.where(hit, (keys >> 32).int().view(torch.float32), torch.zeros((), device=dev)).reshape(N, height, width)
    face = torch.where(hit, (keys & 0xffffffff).int(), torch.full((), -1, dtype=torch.int32, device=dev)).reshape(N, height, width)
    return depth, face, side, behind


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed batch")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    volume = fused_scene(dev)
    fine = volume.mesh_tensors()
    coarse = tuple(torch.from_numpy(a).to(dev) for a in coarse_wall())
    meshes = {"fine": fine, "coarse": coarse, "box": tuple(torch.from_numpy(a).to(dev) for a in box_around())}
    out = {"device": torch.cuda.get_device_name(0), "scene": "fused_scene_256", "image": [H, W], "reps": args.reps, "inner": args.inner,
           "near": NEAR, "shipped_large_box": reconstruction.MESH_RASTER_LARGE_BOX,
           "meshes": {name: {"vertices": int(v.shape[0]), "faces": int(f.shape[0])} for name, (v, f) in meshes.items()},
           "timing": "HIP events around batches of op calls after warm-up: [median, min, max] ms per call"}

    def timed(fn):
        return [round(t, 4) for t in median_ms(fn, args.reps, args.inner)]

    cameras = {}
    for n in (1, 16):
        P = torch.from_numpy(views(n)).to(dev)
        cameras[n] = (torch.from_numpy(np.repeat(K[None], n, axis=0)).to(dev), P)

    out["ops"], out["sweep"], checks = {}, {}, {"sweep_equal_bitwise": True}
    for name, (verts, faces) in meshes.items():
        for n, (Kt, P) in cameras.items():
            tag = f"{name}_N{n}"
            depth, face, overflow = ops.mesh_raster(verts, faces, Kt, P, H, W, near=NEAR, return_overflow=True)
            out["ops"][tag] = {"mesh_raster_ms": timed(lambda: ops.mesh_raster(verts, faces, Kt, P, H, W, near=NEAR)),
                               "mesh_visibility_ms": timed(lambda: ops.mesh_visibility(verts, depth, Kt, P, near=NEAR)),
                               "pixels_hit": round(float((face >= 0).float().mean()), 4), "overflow": int(overflow.sum())}
            out["sweep"][tag] = {}
            for box in SWEEP:
                d, f = ops.mesh_raster(verts, faces, Kt, P, H, W, near=NEAR, large_box=box)
                checks["sweep_equal_bitwise"] &= bool(torch.equal(d.view(torch.int32), depth.view(torch.int32)) and torch.equal(f, face))
                out["sweep"][tag][str(box)] = timed(lambda: ops.mesh_raster(verts, faces, Kt, P, H, W, near=NEAR, large_box=box))

    out["eager"] = {}
    verts, faces = fine
    for n, (Kt, P) in cameras.items():
        w2c = reconstruction.mesh_raster_cameras(P)
        depth, face = ops.mesh_raster(verts, faces, Kt, P, H, W, near=NEAR)
        e_depth, e_face, side, behind = eager_raster(verts, faces, Kt, w2c, H, W)
        checks[f"eager_equal_bitwise_N{n}"] = bool(torch.equal(e_depth.view(torch.int32), depth.view(torch.int32)) and torch.equal(e_face, face))
        checks[f"eager_pixels_differing_N{n}"] = int(((e_depth.view(torch.int32) != depth.view(torch.int32)) | (e_face != face)).sum())
        checks[f"eager_vertices_behind_near_N{n}"] = behind
        out["eager"][f"fine_N{n}"] = {"mesh_raster_ms": timed(lambda: eager_raster(verts, faces, Kt, w2c, H, W)) if n == 1 else
                                      [round(t, 4) for t in median_ms(lambda: eager_raster(verts, faces, Kt, w2c, H, W), max(args.reps // 4, 3), 1)],
                                      "largest_box_side": side}
    out["eager_over_ops"] = {tag: round(out["eager"][tag]["mesh_raster_ms"][0] / out["ops"][tag]["mesh_raster_ms"][0], 2) for tag in out["eager"]}

    Kt, P = cameras[16]
    cast = volume.render(Kt, P, H, W, normals=False, colour=False)[0]
    drawn = render_mesh(verts, faces, Kt, P, H, W, near=NEAR)[0]
    both = (cast > 0) & (drawn > 0)
    difference = (cast - drawn).abs()[both] / 0.01
    out["renderers"] = {"pixels_hit_by_both": round(float(both.float().mean()), 4),
                        "median_abs_difference_voxels": round(float(difference.median()), 5),
                        "p99_abs_difference_voxels": round(float(torch.quantile(difference[:: max(difference.numel() // 1000000, 1)], 0.99)), 5)}
    out["checks"] = checks
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    if not all(v for k, v in checks.items() if k.endswith("bitwise") or "bitwise_N" in k):
        raise SystemExit("the rasteriser disagrees with itself or with the eager route")


if __name__ == "__main__":
    main()

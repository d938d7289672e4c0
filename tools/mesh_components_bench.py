"""Device time of mesh cleaning (csrc/mesh_components.hip) on the mesh of the ``fused_scene_256`` volume of tools/marching_cubes_bench.py,
as it is extracted and with 1 000 small blobs (octahedra of 8 faces) added to it, the floaters the step exists to remove.

hip      ``dvmvs.hip.components.mesh_components`` (the labelling with counts and areas: six launches, no host read) and
         ``filter_components`` (the whole filter: labelling, decision, scans, the one host read, compaction), with ``min_faces=100``.
eager    the same definition in eager torch on the device: labels hooked to the smaller label of every edge with ``scatter_reduce`` (amin)
         and chains followed by ``labels[labels]``, until a DOWNLOADED flag says nothing changed; counts by ``bincount``, areas by
         ``index_add_`` of the float64 formula's integers, compaction by boolean masks and a cumulative sum.
scipy    ``scipy.sparse.csgraph.connected_components`` on the host with the download of the faces (labels canonicalised to the smallest
         index); the whole filter with numpy for the rest and the download of the vertices.
The three give equal labels and equal kept faces (checked before anything is timed).  HIP events around each call after warm-up for the
device paths, wall time for the host path: [median, min, max] ms over ``--reps`` calls.  Prints one JSON line; ``--out PATH`` writes it.

    python tools/mesh_components_bench.py [--reps 10] [--out profiles/mesh_components_bench.json]
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

from dvmvs.components import ComponentFilter  # noqa: E402
from dvmvs.hip import components  # noqa: E402
from dvmvs.tsdf import marching_cubes  # noqa: E402
from marching_cubes_bench import fused_scene  # noqa: E402
from tsdf_fuse_bench import median_ms  # noqa: E402

RULE = ComponentFilter(min_faces=100)
OCTAHEDRON = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])


def with_blobs(verts, faces, n, seed=0):
    """The mesh with ``n`` octahedra of 1 cm appended, scattered over the volume."""
    rng = np.random.default_rng(seed)
    corners = 0.01 * np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float32)
    centres = rng.uniform([-1.2, -1.2, 0.1], [1.2, 1.2, 2.4], (n, 3)).astype(np.float32)
    more_verts = (centres[:, None, :] + corners[None]).reshape(-1, 3)
    more_faces = (OCTAHEDRON[None] + 6 * np.arange(n)[:, None, None] + verts.shape[0]).reshape(-1, 3).astype(np.int32)
    dev = verts.device
    return torch.cat([verts, torch.from_numpy(more_verts).to(dev)]), torch.cat([faces, torch.from_numpy(more_faces).to(dev)])


def eager_labels(faces, V):
    """(labels int64 [V], the number of downloaded flags)."""
    index = faces.long()
    valid = ((index >= 0) & (index < V)).all(dim=1)
    good = index[valid]
    e0, e1 = torch.cat([good[:, 0], good[:, 1]]), torch.cat([good[:, 1], good[:, 2]])
    labels = torch.arange(V, device=faces.device)
    flags = 0
    while True:
        la, lb = labels[e0], labels[e1]
        low = torch.minimum(la, lb)
        hooked = labels.scatter_reduce(0, la, low, "amin").scatter_reduce(0, lb, low, "amin")
        for _ in range(4):                                       # (a few jumps per flag: the flag decides, not their number)
            hooked = hooked[hooked]
        flags += 1
        if not bool((hooked != labels).any()):                   # the download
            return labels, flags
        labels = hooked


def eager_filter(verts, faces):
    V = verts.shape[0]
    labels, _ = eager_labels(faces, V)
    index = faces.long()
    valid = ((index >= 0) & (index < V)).all(dim=1)
    face_labels = torch.where(valid, labels[index[:, 0].clamp(0, V - 1)], torch.full_like(index[:, 0], -1))
    face_count = torch.bincount(face_labels[valid], minlength=V)
    a, b, c = (verts[index[:, j].clamp(0, V - 1)].double() for j in range(3))
    e1, e2 = b - a, c - a
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    units = torch.where(valid, (torch.sqrt((cx * cx + cy * cy) + cz * cz) * 0.5 * 4294967296.0).round().long(), torch.zeros_like(index[:, 0]))
    area = torch.zeros(V, dtype=torch.int64, device=verts.device).index_add_(0, face_labels.clamp(min=0), units)
    keep = (face_count > 0) & (face_count >= RULE.min_faces) & (area >= 0)
    face_kept = valid & keep[face_labels.clamp(min=0)]
    vertex_kept = keep[labels]
    new_index = torch.cumsum(vertex_kept.long(), 0) - 1
    return verts[vertex_kept], new_index[index[face_kept]].int(), labels


def scipy_labels(faces, V):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    f = faces.cpu().numpy().astype(np.int64)                     # the download
    good = f[np.all((f >= 0) & (f < V), axis=1)]
    rows, cols = np.concatenate([good[:, 0], good[:, 1]]), np.concatenate([good[:, 1], good[:, 2]])
    n, found = connected_components(coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(V, V)).tocsr(), directed=False)
    smallest = np.full(n, V, dtype=np.int64)
    np.minimum.at(smallest, found, np.arange(V))
    return smallest[found], f


def scipy_filter(verts, faces):
    V = verts.shape[0]
    labels, f = scipy_labels(faces, V)
    host_verts = verts.cpu().numpy()                             # the download
    valid = np.all((f >= 0) & (f < V), axis=1)
    face_labels = np.where(valid, labels[np.clip(f[:, 0], 0, V - 1)], -1)
    face_count = np.bincount(face_labels[valid], minlength=V)
    keep = face_count >= max(RULE.min_faces, 1)
    face_kept = valid & keep[np.maximum(face_labels, 0)]
    vertex_kept = keep[labels]
    new_index = np.cumsum(vertex_kept) - 1
    return host_verts[vertex_kept], new_index[f[face_kept]].astype(np.int32), labels


def wall_ms(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        start = time.perf_counter()
        fn()
        times.append(1000.0 * (time.perf_counter() - start))
    return [round(float(np.median(times)), 4), round(float(np.min(times)), 4), round(float(np.max(times)), 4)]


def measure(verts, faces, reps):
    V, F = int(verts.shape[0]), int(faces.shape[0])
    parts = components.mesh_components(faces, V, verts)
    kept_verts, kept_faces, _, _ = components.filter_components(verts, faces, RULE)
    labels = parts["labels"].cpu().numpy()
    eager_verts, eager_faces, eager = eager_filter(verts, faces)
    _, flags = eager_labels(faces, V)
    host_verts, host_faces, host = scipy_filter(verts, faces)
    equal = bool(np.array_equal(labels, eager.cpu().numpy()) and np.array_equal(labels, host)
                 and torch.equal(kept_faces, eager_faces) and torch.equal(kept_verts, eager_verts)
                 and np.array_equal(kept_faces.cpu().numpy(), host_faces) and np.array_equal(kept_verts.cpu().numpy(), host_verts))
    return {"vertices": V, "faces": F, "components": int(parts["n_components"]), "kept_faces": int(kept_faces.shape[0]),
            "kept_vertices": int(kept_verts.shape[0]), "equal_results": equal,
            "hip": {"labelling_ms": median_ms(lambda: components.mesh_components(faces, V, verts), reps),
                    "whole_filter_ms": median_ms(lambda: components.filter_components(verts, faces, RULE), reps)},
            "eager_torch": {"downloaded_flags": flags, "labelling_ms": median_ms(lambda: eager_labels(faces, V), reps),
                            "whole_filter_ms": median_ms(lambda: eager_filter(verts, faces), reps)},
            "scipy_host": {"labelling_with_download_ms": wall_ms(lambda: scipy_labels(faces, V), reps),
                           "whole_filter_with_download_ms": wall_ms(lambda: scipy_filter(verts, faces), reps)}}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--blobs", type=int, default=1000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    tsdf, _ = fused_scene(dev)
    verts, faces, _, _ = marching_cubes(tsdf, 0.0)
    out = {"device": torch.cuda.get_device_name(0), "scene": "fused_scene_256", "reps": args.reps, "filter": "min_faces=100",
           "timing": "[median, min, max] ms: HIP events around each call after warm-up; wall time for the host path",
           "mesh": measure(verts, faces, args.reps), f"mesh_with_{args.blobs}_blobs": measure(*with_blobs(verts, faces, args.blobs), args.reps)}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

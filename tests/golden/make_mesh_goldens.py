"""Generates tests/golden/tsdf_mesh.npz: the reference reconstruction script's own mesh / point-cloud post-processing.

Like make_goldens.tsdf_goldens, the script (sample-data/run-tsdf-reconstruction.py) is loaded where it lies, with stand-ins for
its absent imports (numba.njit -> identity; cv2 / path from reference_import).  scikit-image is absent too: its
``measure.marching_cubes_lewiner`` is replaced by tests/marching_cubes_cpu.py (index-space output, float32), so what is pinned
is everything the reference does AROUND marching cubes -- world coordinates, colour look-up and decoding, the point cloud, the
two .ply writers, ``calculate_volume_bounds`` -- run by the reference's code on the reference's fused volume (tsdf.npz, frame 1).

    python tests/golden/make_mesh_goldens.py        (build container only: needs the reference tree)
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (TESTS, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import marching_cubes_cpu as mc  # noqa: E402
import synthetic as syn  # noqa: E402
from reference_import import REFERENCE_ROOT, import_reference  # noqa: E402

SCRIPT = os.path.join(REFERENCE_ROOT, "sample-data", "run-tsdf-reconstruction.py")


def load_script():
    import_reference()                       # cv2 / path stand-ins and the reference's dvmvs package the script imports
    numba = types.ModuleType("numba")
    numba.njit = lambda *a, **k: (a[0] if a and callable(a[0]) else (lambda f: f))
    numba.prange = range
    sk = types.ModuleType("skimage")
    sk.measure = types.ModuleType("skimage.measure")

    def marching_cubes_lewiner(volume, level=0):
        verts, faces, normals, _ = mc.marching_cubes(volume, level)
        vals = np.zeros(len(verts), np.float32)
        return verts.astype(np.float32), faces, normals, vals

    sk.measure.marching_cubes_lewiner = marching_cubes_lewiner
    sys.modules.update({"numba": numba, "skimage": sk, "skimage.measure": sk.measure})
    spec = importlib.util.spec_from_file_location("ref_tsdf_mesh", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.FUSION_GPU_MODE == 0
    return mod


def main():
    mod = load_script()
    fused = np.load(os.path.join(HERE, "tsdf.npz"))
    frames, bounds, voxel = syn.tsdf_inputs()
    vol = mod.TSDFVolume(bounds.copy(), voxel, use_gpu=False)
    assert tuple(vol._vol_dim) == tuple(fused["vol_dim"])
    vol._tsdf_vol_cpu = fused["tsdf1"].copy()
    vol._color_vol_cpu = fused["color1"].copy()
    verts, faces, norms, colors = vol.get_mesh()
    pc = vol.get_point_cloud()
    with tempfile.TemporaryDirectory() as tmp:
        mesh_path, pc_path = os.path.join(tmp, "mesh.ply"), os.path.join(tmp, "pc.ply")
        mod.TSDFFusion.meshwrite(mesh_path, verts, faces, norms, colors)
        mod.TSDFFusion.pcwrite(pc_path, pc)
        mesh_ply, pc_ply = open(mesh_path, "rb").read(), open(pc_path, "rb").read()
    depths = [f[1] for f in frames]
    poses = [f[3] for f in frames]
    K = frames[0][2]
    out = dict(tsdf=fused["tsdf1"], color=fused["color1"], vol_origin=vol._vol_origin, voxel_size=np.float64(voxel),
               verts=verts, faces=faces, norms=norms, colors=colors, point_cloud=pc,
               mesh_ply=np.frombuffer(mesh_ply, np.uint8), pc_ply=np.frombuffer(pc_ply, np.uint8),
               bounds=mod.TSDFFusion.calculate_volume_bounds(depths, poses, K))
    path = os.path.join(HERE, "tsdf_mesh.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(verts)} vertices, {len(faces)} faces, {os.path.getsize(path)} bytes; bounds {out['bounds'].tolist()}")


if __name__ == "__main__":
    main()

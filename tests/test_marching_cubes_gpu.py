"""GPU: csrc/marching_cubes.hip (through dvmvs.tsdf.marching_cubes) against the CPU restatement (tests/marching_cubes_cpu.py),
against the reference's post-processing (tests/golden/tsdf_mesh.npz), on large closed surfaces, and end to end through
TSDFVolume.get_mesh and run()."""
import os

import numpy as np
import pytest
import torch

import marching_cubes_cpu as mc
import synthetic as syn
from test_marching_cubes import check_closed, noise_volume, sphere, torus

pytestmark = pytest.mark.gpu


def hip_mesh(vol, device, **kw):
    if "color" in kw and kw["color"] is not None:
        kw["color"] = torch.from_numpy(kw["color"]).to(device)
    from dvmvs.tsdf import marching_cubes
    v, f, n, c = marching_cubes(torch.from_numpy(vol).to(device), **kw)
    return v.cpu().numpy(), f.cpu().numpy(), n.cpu().numpy(), None if c is None else c.cpu().numpy()


def assert_same_mesh(got, exp):
    gv, gf, gn, gc = got
    ev, ef, en, ec = exp
    assert gv.shape == ev.shape and gf.shape == ef.shape
    assert np.array_equal(gv, ev) and np.array_equal(gf, ef)
    np.testing.assert_allclose(gn, en, atol=1e-6, rtol=0)
    assert (gc is None) == (ec is None) and (gc is None or np.array_equal(gc, ec))


def color_volume(shape, seed):
    rgb = np.random.default_rng(seed).integers(0, 256, size=shape + (3,)).astype(np.float32)
    return (rgb[..., 2] * 65536 + rgb[..., 1] * 256 + rgb[..., 0]).astype(np.float32)


@pytest.fixture(scope="module")
def pin(golden_dir):
    return np.load(os.path.join(golden_dir, "tsdf_mesh.npz"))


def test_hip_equals_the_cpu_restatement(hip_device, pin):
    cases = [(pin["tsdf"], dict(level=0.0, color=pin["color"], origin=pin["vol_origin"], voxel_size=float(pin["voxel_size"])))]
    for shape, seed in (((2, 2, 2), 0), ((33, 17, 65), 1), ((1, 8, 8), 2), ((3, 2, 5), 3)):
        vol = noise_volume(shape, seed, border=False)
        cases.append((vol, dict(level=0.1, color=color_volume(shape, seed), origin=(0.5, -1.25, 2.0), voxel_size=0.03)))
    cases.append((noise_volume((33, 17, 65), 4), dict()))
    cases.append((np.full((9, 10, 11), 2.0, np.float32), dict(color=color_volume((9, 10, 11), 5))))      # all outside: empty
    cases.append((sphere(64, 20.0), dict(level=0.0)))
    for vol, kw in cases:
        exp = mc.marching_cubes(vol, **kw)
        got = hip_mesh(vol, hip_device, **kw)
        assert_same_mesh(got, exp)
    assert len(mc.marching_cubes(cases[1][0], **cases[1][1])[1]) > 0          # the 2x2x2 noise cube has a surface
    assert len(mc.marching_cubes(cases[3][0], **cases[3][1])[0]) == 0         # 1x8x8: none


def test_hip_mesh_equals_the_reference_post_processing(hip_device, pin):
    from dvmvs.tsdf import marching_cubes
    dev = hip_device
    v, f, n, c = marching_cubes(torch.from_numpy(pin["tsdf"]).to(dev), 0.0, torch.from_numpy(pin["color"]).to(dev),
                                pin["vol_origin"], float(pin["voxel_size"]))
    v, f, n, c = v.cpu().numpy(), f.cpu().numpy(), n.cpu().numpy(), c.cpu().numpy()
    assert np.array_equal(v, pin["verts"]) and np.array_equal(c, pin["colors"]) and np.array_equal(f, pin["faces"])
    np.testing.assert_allclose(n, pin["norms"], atol=1e-6, rtol=0)
    assert np.array_equal(np.hstack([v, c]), pin["point_cloud"])


@pytest.mark.parametrize("shape,euler", [("sphere", 2), ("torus", 0)])
def test_large_closed_surfaces_are_watertight_and_deterministic(hip_device, shape, euler):
    from dvmvs.tsdf import marching_cubes
    vol = sphere(256, 100.0) if shape == "sphere" else torus(256, 80.0, 30.0)
    dv = torch.from_numpy(vol).to(hip_device)
    first = marching_cubes(dv)
    second = marching_cubes(dv)
    torch.cuda.synchronize()
    for a, b in zip(first[:3], second[:3]):
        assert torch.equal(a, b)
    verts, faces = first[0].cpu().numpy(), first[1].cpu().numpy()
    assert len(faces) > 100000
    assert check_closed(verts, faces) == euler


def ply_counts(path):
    head = open(path, "rb").read().split(b"end_header\n")[0].decode()
    counts = {}
    for line in head.splitlines():
        if line.startswith("element"):
            _, name, n = line.split()
            counts[name] = int(n)
    return counts


def test_tsdf_volume_get_mesh_and_meshwrite(hip_device, tmp_path):
    from dvmvs.tsdf import TSDFFusion, TSDFVolume
    frames, bounds, voxel = syn.tsdf_inputs()
    vol = TSDFVolume(bounds.copy(), voxel, device=hip_device)
    for n, (rgb, depth, K, pose) in enumerate(frames):
        vol.integrate(rgb, depth, K, pose, obs_weight=1.0 + n)
    verts, faces, norms, colors = vol.get_mesh()
    tsdf, color = vol.get_volume()
    exp = mc.marching_cubes(tsdf, 0.0, color, vol._vol_origin, voxel)
    assert_same_mesh((verts, faces, norms, colors), exp)
    assert len(faces) > 100 and verts.dtype == np.float32 and faces.dtype == np.int32 and colors.dtype == np.uint8
    pc = vol.get_point_cloud()
    assert pc.shape == (len(verts), 6) and pc.dtype == np.float32 and np.array_equal(pc[:, :3], verts)
    TSDFFusion.meshwrite(str(tmp_path / "m.ply"), verts, faces, norms, colors)
    TSDFFusion.pcwrite(str(tmp_path / "p.ply"), pc)
    assert ply_counts(tmp_path / "m.ply") == {"vertex": len(verts), "face": len(faces)}
    assert ply_counts(tmp_path / "p.ply") == {"vertex": len(verts)}


def test_run_writes_meshes_from_saved_predictions(hip_device, golden_dir, tmp_path):
    """A two-keyframe scene folder from tests/golden/sample_scene (frames 00012 / 00013 with their depth maps, poses rows 9 / 10);
    the 'predictions' are those depth maps resized to 320x256."""
    from PIL import Image
    from dvmvs.dataset_loader import load_depth_png, resize_nearest
    from dvmvs.tsdf import TSDFFusion, run
    src = os.path.join(golden_dir, "sample_scene")
    scene = tmp_path / "data" / "hololens-dataset" / "000"
    (scene / "images").mkdir(parents=True)
    (scene / "depth").mkdir()
    names = ["00012.png", "00013.png"]
    for name in names:
        Image.open(os.path.join(src, "images", name)).save(scene / "images" / name)
        Image.open(os.path.join(src, "depth", name)).save(scene / "depth" / name)
    poses = np.loadtxt(os.path.join(golden_dir, "hololens_000_poses.txt")).reshape(-1, 16)[[9, 10]]
    np.savetxt(scene / "poses.txt", poses)
    np.savetxt(scene / "K.txt", np.loadtxt(os.path.join(golden_dir, "hololens_000_K.txt")))
    (tmp_path / "data" / "indices").mkdir()
    (tmp_path / "data" / "indices" / "keyframe+hololens-dataset+000+nmeas+3").write_text("00012.png 00009.png\nTRACKING LOST\n00013.png 00012.png\n")
    preds = np.stack([resize_nearest(load_depth_png(os.path.join(src, "depth", n)), 320, 256) for n in names]).astype(np.float32)
    (tmp_path / "pred").mkdir()
    np.savez(tmp_path / "pred" / "keyframe_hololens-dataset_320_256_3_dvmvs_fusionnet_online_predictions_000.npz", preds)
    out = tmp_path / "rec"
    run(str(out), str(tmp_path / "pred"), str(tmp_path / "data"), "hololens-dataset", "000", "320_256_3_dvmvs_fusionnet_online",
        0.05, 5.0, False, False, True, device=hip_device)
    written = sorted(os.listdir(out))
    assert len(written) == 2 and all(w.endswith("_complete.ply") for w in written)
    assert any("GROUNDTRUTH" in w for w in written)
    scaled_K = np.loadtxt(os.path.join(golden_dir, "hololens_000_K.txt"))
    scaled_K[0] *= 320 / 540.0
    scaled_K[1] *= 256 / 360.0
    preds[preds > 5.0] = 0.0
    bounds = 1.05 * TSDFFusion.calculate_volume_bounds(list(preds), list(poses.reshape(-1, 4, 4)), scaled_K)
    for w in written:
        counts = ply_counts(out / w)
        assert counts["vertex"] > 1000 and counts["face"] > 1000
        lines = open(out / w).read().split("end_header\n")[1].splitlines()
        assert len(lines) == counts["vertex"] + counts["face"]
        xyz = np.array([[float(t) for t in line.split()[:3]] for line in lines[:counts["vertex"]]])
        assert (xyz >= bounds[:, 0] - 1e-5).all() and (xyz <= bounds[:, 1] + 0.05 + 1e-5).all()

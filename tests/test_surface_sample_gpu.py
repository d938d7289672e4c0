"""GPU: the device ops of csrc/surface_sample.hip against their host definitions in dvmvs.errors -- points compared as int32 bit patterns --
then ``TSDFVolume.score_against`` with sampling and down-sampling, and ``python -m dvmvs.tsdf`` with the flags that switch them on.  A
host reference is computed once per case and never modified."""
import os

import numpy as np
import pytest
import torch

import nearest_reference as nr
import surface_sample_cases as cases
import tsdf_fuse_scene as scene
from dvmvs import errors

pytestmark = pytest.mark.gpu


def device_samples(dev, verts, faces, density, seed=0):
    from dvmvs.hip import ops
    points, face = ops.surface_sample(torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev), density, seed, return_face=True)
    assert points.is_cuda and points.dtype == torch.float32 and face.dtype == torch.int32 and points.is_contiguous()
    alone = ops.surface_sample(torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev), density, seed)
    assert torch.equal(alone, points)                                              # without the faces: the same points; and run to run
    return points.cpu().numpy(), face.cpu().numpy()


def assert_samples(dev, verts, faces, density, seed=0):
    want_points, want_face = errors.sample_surface(verts, faces, density, seed, return_face=True)
    points, face = device_samples(dev, verts, faces, density, seed)
    print(f"V {len(verts)} F {len(faces)} density {density} seed {seed}: {len(want_points)} samples")
    assert points.shape == want_points.shape and np.array_equal(face, want_face)
    assert np.array_equal(cases.bits(points), cases.bits(want_points))
    return len(want_points)


# ---- surface_sample ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 7])
def test_unit_square(hip_device, seed):
    assert assert_samples(hip_device, *cases.unit_square(), 10000, seed) == 10000


@pytest.mark.parametrize("seed", [0, 7])
def test_soup(hip_device, seed):
    assert assert_samples(hip_device, *cases.soup(), 50, seed) == 70114


def test_single_triangle(hip_device):
    verts = cases.f32([[0.5, -2.0, 1.0], [3.5, 0.25, -1.0], [-1.0, 4.0, 2.5]])
    assert assert_samples(hip_device, verts, np.array([[2, 0, 1]], np.int32), 777.0, 3) > 5000


# the last two: 1024 and 1025 workgroup totals, so every thread of the one-workgroup scan has a total, then chunks of two with a short last one
@pytest.mark.parametrize("F", [1, 255, 256, 257, 1023, 1024, 1025, 70000, 1024 * 1024, 1024 * 1024 + 1])
def test_small_triangles_across_the_scan_blocks(hip_device, F):
    assert assert_samples(hip_device, *cases.small_triangles(F), 300.0) > 2 * F


def test_one_large_triangle_among_tiny_ones(hip_device):
    verts, faces = cases.one_large_among_tiny()
    n = assert_samples(hip_device, verts, faces, 100.0)
    face = errors.sample_surface(verts, faces, 100.0, return_face=True)[1]
    counts = np.bincount(face, minlength=len(faces))
    assert counts[500] > 190000 and counts[500] + 1000 >= n and np.delete(counts, 500).max() <= 1


def test_faces_with_indices_out_of_range_are_ignored(hip_device):
    verts, faces = cases.out_of_range_mesh()
    assert_samples(hip_device, verts, faces, 10000)
    points, face = device_samples(hip_device, verts, faces, 10000)
    assert np.array_equal(points, errors.sample_surface(*cases.unit_square(), 10000)) and set(face.tolist()) == {1, 4}


def test_no_sample(hip_device):
    from dvmvs.hip import ops
    verts, faces = cases.speck()
    points, face = device_samples(hip_device, verts, faces, 1e6)
    assert points.shape == (0, 3) and face.shape == (0,)
    empty = ops.surface_sample(torch.from_numpy(verts).to(hip_device), torch.zeros((0, 3), dtype=torch.int32, device=hip_device), 10.0)
    assert tuple(empty.shape) == (0, 3) and empty.is_cuda
    no_vertex = ops.surface_sample(torch.zeros((0, 3), device=hip_device), torch.from_numpy(faces).to(hip_device), 10.0)
    assert tuple(no_vertex.shape) == (0, 3)


def test_surface_sample_argument_checks(hip_device):
    from dvmvs.hip import ops
    verts, faces = (torch.from_numpy(a).to(hip_device) for a in cases.unit_square())
    for density in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ops.surface_sample(verts, faces, density)
    with pytest.raises(ValueError):
        ops.surface_sample(verts, faces, 1e9)                                       # above 2^28 samples: refused before any allocation
    with pytest.raises(ValueError):
        ops.surface_sample(verts * 1e5, faces, 1.0)                                 # 1e10 m^2
    with pytest.raises(ValueError):
        ops.surface_sample(verts, faces, 10.0, seed=-1)
    with pytest.raises(ValueError):
        ops.surface_sample(verts, faces.to(torch.int64), 10.0)
    with pytest.raises(RuntimeError):
        ops.surface_sample(verts.cpu(), faces.cpu(), 10.0)


# ---- voxel_downsample -------------------------------------------------------------------------------------------------------------------------
def assert_voxels(dev, points, voxel):
    from dvmvs.hip import ops
    want, want_counts = errors.voxel_down_sample(points, voxel, return_counts=True)
    out, counts = ops.voxel_downsample(torch.from_numpy(points).to(dev), voxel, return_counts=True)
    assert out.is_cuda and out.dtype == torch.float32 and counts.dtype == torch.int32
    assert torch.equal(ops.voxel_downsample(torch.from_numpy(points).to(dev), voxel), out)
    out, counts = out.cpu().numpy(), counts.cpu().numpy()
    print(f"{len(points)} points at {voxel}: {len(want)} voxels, largest population {want_counts.max()}")
    assert out.shape == want.shape and np.array_equal(counts, want_counts)
    assert np.array_equal(cases.bits(out), cases.bits(want))
    return len(want)


# the last: 1025 workgroup totals for the one-workgroup scan (chunks of two, the last one short), at a voxel that leaves most points alone
@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000, 50000, 1024 * 1024 + 1])
def test_gaussian_clouds(hip_device, N):
    assert_voxels(hip_device, cases.gaussian(N, 3 if N >= 50000 else N), 0.25 if N <= 50000 else 0.02)


def test_coincident_points(hip_device):
    assert assert_voxels(hip_device, cases.coincident(), 0.25) == 1


def test_points_on_voxel_faces(hip_device):
    assert_voxels(hip_device, cases.on_voxel_faces(), 0.25)


def test_negative_coordinates(hip_device):
    assert_voxels(hip_device, cases.negative_cloud(), 0.3)


def test_voxel_downsample_argument_checks(hip_device):
    from dvmvs.hip import ops
    cloud = torch.from_numpy(cases.gaussian(100, 1)).to(hip_device)
    for voxel in (0.0, -0.25, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ops.voxel_downsample(cloud, voxel)
    with pytest.raises(ValueError):
        ops.voxel_downsample(cloud[:0], 0.25)
    wide = torch.tensor([[0.0, 0.0, 0.0], [0.0, 2 ** 21 * 0.25, 0.0]], device=hip_device)
    with pytest.raises(ValueError):
        ops.voxel_downsample(wide, 0.25)                                            # cell 2^21 on y
    assert tuple(ops.voxel_downsample(wide * ((2 ** 21 - 1) / 2 ** 21), 0.25).shape) == (2, 3)
    assert_voxels(hip_device, cases.gaussian(100, 1), 0.25)                         # the workspace is in order after a refused cloud
    with pytest.raises(RuntimeError):
        ops.voxel_downsample(cloud.cpu(), 0.25)


# ---- TSDFVolume.score_against -------------------------------------------------------------------------------------------------------------------
def fused(dev, voxel):
    from dvmvs.tsdf import TSDFVolume
    depth, rgb = scene.frames()
    vol = TSDFVolume(scene.BOUNDS.copy(), voxel, device=dev)
    vol.integrate_frames(rgb, depth, scene.K, scene.poses())
    return vol


def test_score_against_two_voxel_sizes(hip_device):
    from dvmvs.hip import ops
    coarse, fine = fused(hip_device, scene.VOXEL), fused(hip_device, 0.04)
    (pv, pf), (gv, gf) = (tuple(t.cpu().numpy() for t in vol.mesh_tensors()) for vol in (coarse, fine))
    assert len(pv) > 100 and len(gv) > len(pv) and pf.dtype == np.int32
    density, voxel = 2000.0, 0.05
    pred, gt = errors.prepare_points(pv, pf, density, voxel), errors.prepare_points(gv, gf, density, voxel)
    for vol, want in ((coarse, pred), (fine, gt)):
        assert np.array_equal(cases.bits(vol.surface_points(density, voxel).cpu().numpy()), cases.bits(want))
    assert np.array_equal(cases.bits(coarse.surface_points(density).cpu().numpy()), cases.bits(errors.sample_surface(pv, pf, density)))
    assert np.array_equal(coarse.surface_points().cpu().numpy(), pv)
    want = errors.compute_reconstruction_errors(pv, gv, 0.05, pred_faces=pf, gt_faces=gf, sample_density=density, voxel=voxel)
    assert np.array_equal(want, errors.compute_reconstruction_errors(pred, gt, 0.05))
    row, sizes = coarse.score_against(fine, 0.05, return_sizes=True, sample_density=density, voxel=voxel)
    row = row.cpu().numpy()
    print(f"{len(pv)} / {len(gv)} vertices -> {sizes} points: device {row}, host {want}")
    assert sizes == (len(pred), len(gt))
    for query, target in ((pred, gt), (gt, pred)):                                 # the distances: bit-identical
        dist = ops.nearest_distance(torch.from_numpy(query).to(hip_device), torch.from_numpy(target).to(hip_device)).cpu().numpy()
        assert np.array_equal(cases.bits(dist), cases.bits(errors.nearest_distances(query, target)))
    # the row: equal but for the last float32 bit of a mean (the fp64 sum in the kernel's order against fsum)
    assert (nr.ulps(row[:3], want[:3]) <= 1).all() and np.array_equal(row[3:5], want[3:5]) and nr.ulps(row[5], want[5]) <= 1
    # the same through the other forms of a reference: a mesh pair on the device, on the host; the device function with its keywords
    for reference in (fine.mesh_tensors(), (gv, gf)):
        assert np.array_equal(coarse.score_against(reference, 0.05, sample_density=density, voxel=voxel).cpu().numpy(), row)
    (dpv, dpf), (dgv, dgf) = coarse.mesh_tensors(), fine.mesh_tensors()
    dev_row = errors.compute_reconstruction_errors_device(dpv, dgv, 0.05, pred_faces=dpf, gt_faces=dgf, sample_density=density, voxel=voxel)
    assert np.array_equal(dev_row.cpu().numpy(), row)
    # a reference that is a point cloud is not sampled, only down-sampled
    cloud_row = coarse.score_against(gv, 0.05, sample_density=density, voxel=voxel).cpu().numpy()
    cloud_want = errors.compute_reconstruction_errors(pred, errors.voxel_down_sample(gv, voxel), 0.05)
    assert (nr.ulps(cloud_row[:3], cloud_want[:3]) <= 1).all() and np.array_equal(cloud_row[3:5], cloud_want[3:5])
    # no new argument: today's vertex path, whatever form the reference has
    plain = coarse.score_against(fine).cpu().numpy()
    vertices = errors.compute_reconstruction_errors(pv, gv, 0.05)
    assert (nr.ulps(plain[:3], vertices[:3]) <= 1).all() and np.array_equal(plain[3:5], vertices[3:5])
    assert np.array_equal(coarse.score_against(gv).cpu().numpy(), plain) and np.array_equal(coarse.score_against((gv, gf)).cpu().numpy(), plain)
    assert not np.array_equal(plain, row)


# ---- the program --------------------------------------------------------------------------------------------------------------------------------
def test_program_scores_on_sampled_surfaces(hip_device, golden_dir, tmp_path):
    """``python -m dvmvs.tsdf --evaluate_3d`` with ``--evaluate_3d_density`` / ``--evaluate_3d_voxel``, and with ``--groundtruth_mesh``, on two
    keyframes of the sample scene (their depth maps as 'predictions', 5 cm voxels)."""
    from PIL import Image
    from dvmvs.dataset_loader import load_depth_png, resize_nearest
    from dvmvs.errors import RECONSTRUCTION_METRICS
    from dvmvs.tsdf import TSDFFusion, main
    src = os.path.join(golden_dir, "sample_scene")
    scene_dir = tmp_path / "data" / "hololens-dataset" / "000"
    (scene_dir / "images").mkdir(parents=True)
    (scene_dir / "depth").mkdir()
    names = ["00012.png", "00013.png"]
    for name in names:
        Image.open(os.path.join(src, "images", name)).save(scene_dir / "images" / name)
        Image.open(os.path.join(src, "depth", name)).save(scene_dir / "depth" / name)
    np.savetxt(scene_dir / "poses.txt", np.loadtxt(os.path.join(golden_dir, "hololens_000_poses.txt")).reshape(-1, 16)[[9, 10]])
    np.savetxt(scene_dir / "K.txt", np.loadtxt(os.path.join(golden_dir, "hololens_000_K.txt")))
    (tmp_path / "data" / "indices").mkdir()
    (tmp_path / "data" / "indices" / "keyframe+hololens-dataset+000+nmeas+3").write_text("00012.png 00009.png\nTRACKING LOST\n00013.png 00012.png\n")
    preds = np.stack([resize_nearest(load_depth_png(os.path.join(src, "depth", n)), 320, 256) for n in names]).astype(np.float32)
    (tmp_path / "pred").mkdir()
    np.savez(tmp_path / "pred" / "keyframe_hololens-dataset_320_256_3_dvmvs_fusionnet_online_predictions_000.npz", preds)
    common = ["--prediction_folder", str(tmp_path / "pred"), "--data_folder", str(tmp_path / "data"), "--voxel_size", "0.05", "--evaluate_3d",
              "--threshold_3d", "0.1"]

    def run(tag, flags):
        out = tmp_path / tag
        main(["--reconstruction_folder", str(out)] + common + flags)
        files = sorted(os.listdir(out))
        errors_file, = [w for w in files if w.endswith("_errors3d.npz")]
        return out, files, np.load(out / errors_file)

    out, files, saved = run("sampled", ["--evaluate_3d_density", "2000", "--evaluate_3d_voxel", "0.05"])
    assert len(files) == 2                                                         # the system's mesh and the errors: no ground-truth mesh
    mesh_file, = [w for w in files if w.endswith("_complete.ply")]
    row, counts, points = saved["arr_0"], saved["counts"], saved["points"]
    print(f"sampled: {dict(zip(RECONSTRUCTION_METRICS, row.tolist()))}, vertices {counts}, points {points}")
    assert tuple(saved["names"].tolist()) == RECONSTRUCTION_METRICS and saved["threshold"] == np.float32(0.1)
    assert saved["sample_density"] == 2000.0 and saved["voxel"] == 0.05
    assert row.dtype == np.float32 and row.shape == (6,) and np.isfinite(row).all() and (row[:3] >= 0).all() and ((row[3:] >= 0) & (row[3:] <= 1)).all()
    assert counts.dtype == np.int64 and points.dtype == np.int64 and counts.shape == points.shape == (2,) and (points > 0).all()
    verts, faces = TSDFFusion.meshread(str(out / mesh_file))
    assert len(verts) == counts[0]

    # against a mesh file: the system's own mesh, written again by the test; nothing of the ground-truth depth is fused
    mesh_path = str(tmp_path / "groundtruth.ply")
    TSDFFusion.meshwrite(mesh_path, verts, faces, np.zeros_like(verts), np.zeros((len(verts), 3), np.uint8))
    for tag, flags, density, voxel in (("mesh", [], None, None), ("mesh_sampled", ["--evaluate_3d_density", "2000", "--evaluate_3d_voxel", "0.05"], 2000.0, 0.05)):
        out, files, saved = run(tag, ["--groundtruth_mesh", mesh_path] + flags)
        assert len(files) == 2
        row = saved["arr_0"]
        print(f"{tag}: {dict(zip(RECONSTRUCTION_METRICS, row.tolist()))}, vertices {saved['counts']}, points {saved['points']}")
        assert saved["counts"].tolist() == [len(verts), len(verts)]
        assert row[3] == 1 and row[4] == 1 and row[5] == 1 and row[2] < 1e-3        # the same surface, to the six decimals of the file
        if density is None:
            assert np.isnan(saved["sample_density"]) and np.isnan(saved["voxel"]) and saved["points"].tolist() == [len(verts), len(verts)]
        else:
            assert saved["sample_density"] == density and saved["voxel"] == voxel and (saved["points"] > 0).all()
    with pytest.raises(ValueError):
        main(["--reconstruction_folder", str(tmp_path / "refused"), "--prediction_folder", str(tmp_path / "pred"), "--data_folder",
              str(tmp_path / "data"), "--evaluate_3d_voxel", "0.05"])

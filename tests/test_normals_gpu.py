"""GPU: oriented point normals on the device (csrc/point_normals.hip through dvmvs/hip/normals.py) against the host definition
(dvmvs/normals.py), bit for bit: normals, curvature and valid of every case of tests/normals_cases.py, alignment, streams, a cloud of many
workgroups, and the program's ``--point_normals_*`` flags."""
import functools
import os

import numpy as np
import pytest
import torch

import consistency_reference as cr
import normals_cases as cases
from dvmvs import normals as nm
from dvmvs.outliers import nearest_neighbours

pytestmark = pytest.mark.gpu

SEARCH = cases.search_cases()
ROWS = cases.row_cases()


def upload(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def same_bits(got, want):
    """``(normals, curvature, valid)`` of the device against the host's: dtypes, shapes and every bit."""
    assert len(got) == len(want) == 3
    for name, g, w in zip(("normals", "curvature", "valid"), got, want):
        g = g.cpu().numpy() if torch.is_tensor(g) else g
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, g.shape, w.dtype, w.shape)
        if g.tobytes() != w.tobytes():
            rows = np.flatnonzero((g.reshape(len(g), -1).view(np.uint8) != w.reshape(len(w), -1).view(np.uint8)).any(axis=1))
            raise AssertionError(f"{name}: {len(rows)} of {len(g)} rows differ, first {rows[0]}: {g[rows[0]]} != {w[rows[0]]}")


@functools.lru_cache(maxsize=None)
def host_search(name):
    points, k, limit, viewpoints, view = SEARCH[name]
    return nm.estimate_normals(points, k, limit, viewpoints, view)


@pytest.mark.parametrize("name", list(SEARCH))
def test_clouds_against_themselves(hip_device, name):
    points, k, limit, viewpoints, view = SEARCH[name]
    want = host_search(name)
    got = nm.estimate_normals_device(upload(hip_device, points), k, limit, upload(hip_device, viewpoints), upload(hip_device, view))
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.float32 and got[2].dtype == torch.bool
    same_bits(got, want)
    if name.startswith("sphere") and "-bounded" in name and k >= 20:
        index = nearest_neighbours(points, points, k, limit)[1]
        assert (index < 0).any() and want[2].all()                                   # rows with missing slots, still three neighbours
    if name in ("duplicates", "collinear"):
        assert want[2].sum() == (0 if name == "duplicates" else len(points))
    if name == "blob-and-far-points":
        assert (~want[2]).sum() == 20
    if name.startswith("gaussian-n") and len(points) < 3:
        assert not want[2].any()


@pytest.mark.parametrize("name", list(ROWS))
def test_given_rows(hip_device, name):
    """Separate clouds, and hand-made rows with -1 in the middle and slots outside [0, M) (M, 2^31 - 1, -7), through the binding: the
    outputs equal the host form's (a slot outside that were read would change them) and the arguments are left as they were."""
    from dvmvs.hip import normals as binding
    points, target, index, viewpoints, view = ROWS[name]
    want = nm.point_normals(points, target, index, viewpoints, view)
    dev = [upload(hip_device, a) for a in (points, target, index, viewpoints, view)]
    got = binding.point_normals(*dev)
    same_bits(got, want)
    for before, after in zip((points, target, index, viewpoints, view), dev):
        assert before is None or np.array_equal(after.cpu().numpy(), before)
    if name == "hand-made-rows":
        assert want[2].tolist() == [True] * 26 + [False] * 4 + [True] * 10        # two slots, none, one, one place eight times
        # the target between eight rows of NaN on either side: a slot of M or -7 that were read would bring one into the sums
        M = len(target)
        padded = torch.full((M + 16, 3), float("nan"), device=hip_device)
        padded[8:8 + M] = dev[1]
        same_bits(binding.point_normals(dev[0], padded[8:8 + M], dev[2], dev[3], dev[4]), want)


def test_alignment_and_layout(hip_device):
    """Tensors that are 4-byte and not 16-byte aligned (a storage offset of one element), and inputs that are not contiguous."""
    from dvmvs.hip import normals as binding
    points, target, index, viewpoints, view = ROWS["separate-clouds"]
    want = nm.point_normals(points, target, index, viewpoints, view)

    def shifted(a):
        a = upload(hip_device, a)
        buffer = torch.zeros(a.numel() + 5, dtype=a.dtype, device=hip_device)
        out = buffer[1:1 + a.numel()].view(a.shape)
        out.copy_(a)
        assert out.data_ptr() % 8 == 4 and out.is_contiguous()
        return out

    same_bits(binding.point_normals(*(shifted(a) for a in (points, target, index, viewpoints, view))), want)

    def strided(a):
        a = upload(hip_device, a)
        wide = torch.zeros(a.shape[:-1] + (2 * a.shape[-1],), dtype=a.dtype, device=hip_device)
        out = wide[..., ::2]
        out.copy_(a)
        assert not out.is_contiguous()
        return out

    same_bits(binding.point_normals(*(strided(a) for a in (points, target, index, viewpoints, view))), want)
    # the xyz columns of an xyzrgb cloud, as the program passes them
    cloud = torch.cat([upload(hip_device, points), torch.rand((len(points), 3), device=hip_device)], dim=1)
    same_bits(binding.point_normals(cloud[:, :3], upload(hip_device, target), upload(hip_device, index), upload(hip_device, viewpoints),
                                    upload(hip_device, view)), want)


def test_many_workgroups(hip_device):
    """70 001 points at k = 8: not a multiple of 256.  The rows are the device search's (a brute force of this size is not for the host);
    the host form gets the same rows."""
    from dvmvs.hip import neighbours
    points = cases.sheet()
    viewpoints = np.array([[1.5, 1.0, 4.0]], np.float32)
    q = upload(hip_device, points)
    got = nm.estimate_normals_device(q, 8, 0.05, upload(hip_device, viewpoints))
    index = neighbours.knn(q, q, 8, 0.05)[1].cpu().numpy()
    assert (index[:, 0] == np.arange(len(points))).all()
    want = nm.point_normals(points, points, index, viewpoints)
    same_bits(got, want)
    assert want[2].all() and (want[0][:, 2] > 0.9).all()                            # the sheet faces the viewpoint above it


def test_repeatable_on_any_stream_and_with_a_given_grid(hip_device):
    from dvmvs.hip import normals as binding, ops
    points, k, limit, viewpoints, view = SEARCH["sphere-k20-bounded-three"]
    want = host_search("sphere-k20-bounded-three")
    q, vp, vw = upload(hip_device, points), upload(hip_device, viewpoints), upload(hip_device, view)
    first = binding.estimate_normals(q, k, limit, vp, vw)
    second = binding.estimate_normals(q, k, limit, vp, vw)
    with_grid = binding.estimate_normals(q, k, limit, vp, vw, grid=ops.nearest_build(q))
    side = torch.cuda.Stream(device=hip_device)
    side.wait_stream(torch.cuda.current_stream(hip_device))
    with torch.cuda.stream(side):
        third = binding.estimate_normals(q, k, limit, vp, vw)
    side.synchronize()
    torch.cuda.current_stream(hip_device).wait_stream(side)
    for other in (first, second, with_grid, third):
        same_bits(other, want)


def test_empty_cloud_and_argument_checks(hip_device):
    from dvmvs.hip import normals as binding
    empty = torch.zeros((0, 3), device=hip_device)
    q = torch.rand((6, 3), device=hip_device)
    index = torch.zeros((6, 4), dtype=torch.int32, device=hip_device)
    for got in (binding.estimate_normals(empty), binding.point_normals(empty, q, torch.zeros((0, 4), dtype=torch.int32, device=hip_device))):
        assert got[0].shape == (0, 3) and got[1].shape == (0,) and got[2].shape == (0,) and got[2].dtype == torch.bool
    with pytest.raises(ValueError, match="empty"):
        binding.point_normals(q, empty, index)
    with pytest.raises(ValueError, match="index"):
        binding.point_normals(q, q, index.long())
    with pytest.raises(ValueError, match="index"):
        binding.point_normals(q, q, index[:5])
    with pytest.raises(ValueError, match="view"):
        binding.point_normals(q, q, index, torch.zeros((2, 3), device=hip_device))
    with pytest.raises(ValueError, match="viewpoints"):
        binding.point_normals(q, q, index, None, torch.zeros(6, dtype=torch.int32, device=hip_device))
    with pytest.raises(ValueError, match="view"):
        binding.point_normals(q, q, index, torch.zeros((2, 3), device=hip_device), torch.zeros(5, dtype=torch.int32, device=hip_device))
    with pytest.raises(ValueError, match="max_distance"):
        binding.estimate_normals(q, 3, -1.0)


# ---- the program --------------------------------------------------------------------------------------------------------------------
def write_scene(tmp_path, depths, Ks, poses, system):
    """Five keyframes of the analytic scene of the consistency tests as the folders ``python -m dvmvs.tsdf`` reads."""
    from PIL import Image
    h, w = depths.shape[1:]
    scene_dir = tmp_path / "data" / "hololens-dataset" / "000"
    (scene_dir / "images").mkdir(parents=True)
    rng = np.random.default_rng(5)
    names = [f"{i:05d}.png" for i in range(len(depths))]
    for name in names:
        Image.fromarray(rng.integers(0, 256, (h, w, 3)).astype(np.uint8)).save(scene_dir / "images" / name)
    np.savetxt(scene_dir / "poses.txt", poses.reshape(-1, 16).astype(np.float64))
    np.savetxt(scene_dir / "K.txt", Ks[0].astype(np.float64))
    (tmp_path / "data" / "indices").mkdir()
    (tmp_path / "data" / "indices" / "keyframe+hololens-dataset+000+nmeas+3").write_text("\n".join(f"{n} {n}" for n in names) + "\n")
    (tmp_path / "pred").mkdir()
    np.savez(tmp_path / "pred" / f"keyframe_hololens-dataset_{system}_predictions_000.npz", depths)
    return ["--prediction_folder", str(tmp_path / "pred"), "--data_folder", str(tmp_path / "data"), "--voxel_size", "0.05",
            "--filter_consistency", "--save_point_cloud"]


def read_cloud(path):
    header, body = open(path).read().split("end_header\n")
    return header, body.splitlines()


@pytest.mark.parametrize("cleaned", [False, True])
def test_program_writes_the_normals(hip_device, tmp_path, capsys, cleaned):
    """``python -m dvmvs.tsdf --filter_consistency --save_point_cloud --point_normals_*`` on five 24x32 keyframes: ``_pointcloud_normals.ply``
    holds the valid rows of the written cloud (of the cleaned one with ``--clean_points_neighbours``) with the host definition's normals,
    oriented to the keyframes' camera centres, and every other file is what it is without the flags, byte for byte."""
    from dvmvs.consistency import filter_depths, fused_point_cloud, fused_point_views, nearest_sources
    from dvmvs.dataset_loader import PreprocessImage
    from dvmvs.outliers import OutlierFilter, filter_outliers
    from dvmvs.tsdf import main
    depths, Ks, poses = (a[:5] for a in cr.clean_scene("24x32"))
    h, w = depths.shape[1:]
    system = "320_256_3_dvmvs_fusionnet_online"
    common = write_scene(tmp_path, depths, Ks, poses, system)
    normal_flags = ["--point_normals_neighbours", "10", "--point_normals_max_distance", "0.15"]
    if cleaned:
        common = ["--clean_points_neighbours", "8", "--clean_points_ratio", "1.0", "--clean_points_max_distance", "0.5"] + common
    main(["--reconstruction_folder", str(tmp_path / "plain")] + common)
    capsys.readouterr()
    main(["--reconstruction_folder", str(tmp_path / "normals")] + normal_flags + common)
    printed = capsys.readouterr().out

    stem = f"reconstruction_voxelsize-0.05_maxdepth-5.0_anchor-False_{system}+consistent_hololens-dataset_000"
    before = sorted(os.listdir(tmp_path / "plain"))
    assert before == sorted(stem + end for end in ["_complete.ply", "_pointcloud.ply"] + (["_pointcloud_clean.ply"] if cleaned else []))
    assert sorted(os.listdir(tmp_path / "normals")) == sorted(before + [stem + "_pointcloud_normals.ply"])
    for name in before:
        assert open(tmp_path / "plain" / name, "rb").read() == open(tmp_path / "normals" / name, "rb").read(), name

    # the cloud that was written, with its float32 coordinates (the file holds six decimals of them), and its points' keyframes
    scaled_K = PreprocessImage(K=Ks[0], old_width=w, old_height=h, new_width=w, new_height=h, distortion_crop=0,
                               perform_crop=False).get_updated_intrinsics()
    averaged, _, points = filter_depths(depths, scaled_K, poses, nearest_sources(5, 4), min_views=2, average=True, with_points=True,
                                        device=hip_device)
    xyz = fused_point_cloud(averaged, points).cpu().numpy()
    views = fused_point_views(averaged).cpu().numpy()
    centres = np.ascontiguousarray(poses.astype(np.float32)[:, :3, 3])
    header, rows = read_cloud(tmp_path / "normals" / (stem + ("_pointcloud_clean.ply" if cleaned else "_pointcloud.ply")))
    cloud, cloud_views = xyz, views
    if cleaned:
        mask = filter_outliers(xyz, OutlierFilter(neighbours=8, ratio=1.0, max_distance=0.5), return_mask=True)[1]
        cloud, cloud_views = xyz[mask], views[mask]
        assert 0 < mask.sum() < len(xyz)
    assert len(rows) == len(cloud) <= 4000
    normals, _, valid = nm.estimate_normals(cloud, 10, 0.15, centres, cloud_views)
    print(f"{len(cloud)} points, {int(valid.sum())} with a normal")
    assert 0 < valid.sum() <= len(cloud)
    normals_header, normal_rows = read_cloud(tmp_path / "normals" / (stem + "_pointcloud_normals.ply"))
    assert normals_header == header.replace(f"element vertex {len(cloud)}\n", f"element vertex {int(valid.sum())}\n").replace(
        "property float z\n", "property float z\nproperty float nx\nproperty float ny\nproperty float nz\n")
    kept_rows = [row for row, ok in zip(rows, valid) if ok]
    assert [" ".join(r.split()[:3] + r.split()[6:]) for r in normal_rows] == kept_rows
    assert [" ".join(r.split()[3:6]) for r in normal_rows] == ["%f %f %f" % tuple(n) for n in normals[valid]]
    # every normal faces the camera that saw its point
    toward = centres[cloud_views[valid]].astype(np.float64) - cloud[valid].astype(np.float64)
    assert ((normals[valid].astype(np.float64) * toward).sum(axis=1) >= 0).all()
    assert f"Point normals: {100.0 * valid.sum() / len(cloud):.1f} % of the {len(cloud)} points have a valid normal" in printed

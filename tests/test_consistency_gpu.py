"""GPU: the depth-map consistency filter (csrc/depth_consistency.hip) against its numpy restatement (tests/consistency_reference.py), bit for
bit, and its public surface: ``dvmvs.consistency``, ``LiveFusion(min_consistent_views=...)`` and ``dvmvs.tsdf.run(filter_consistency=True)``.
Nothing here has a tolerance except the distance of the program's point cloud from the analytic surface (one voxel)."""
import os

import numpy as np
import pytest
import torch

import consistency_reference as cr
import tsdf_fuse_scene as fuse_scene

pytestmark = pytest.mark.gpu


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def up(dev, *arrays):
    return [torch.as_tensor(np.array(a), device=dev) for a in arrays]        # (a copy: the shared scenes are read-only)


def filtered(dev, depths, K, poses, sources, **kwargs):
    """The op's three outputs as host arrays."""
    from dvmvs.hip import ops
    d, k, p, s = up(dev, depths, K, poses, np.asarray(sources, np.int32).reshape(len(depths), -1))
    depth, count, points = ops.depth_consistency(d, k, p, s, with_points=True, **kwargs)
    return depth.cpu().numpy(), count.cpu().numpy(), points.cpu().numpy()


def assert_equals_restatement(got, depths, K, poses, sources, **kwargs):
    want = cr.depth_consistency(depths, K, poses, sources, **kwargs)
    for name, g in zip(("depth", "count", "points"), got):
        differ = bits(g) != bits(want[name])
        assert same_bits(g, want[name]), f"{name}: {int(differ.sum())} of {differ.size} elements differ from the float32 restatement ({kwargs})"


def wide_sources(n=6, slots=16):
    """16 slots, most of them skipped (-1, the frame itself, an index >= n); the four of cr.SOURCES sit in slots 1, 5, 9 and 14."""
    table = np.full((n, slots), -1, np.int32)
    table[:, 2], table[:, 7] = np.arange(n), n
    table[:, 12] = n + 5
    table[:, [1, 5, 9, 14]] = cr.SOURCES[:n]
    return table


BATCHES = {"1x0": (1, np.zeros((1, 0), np.int32)), "2x1": (2, np.array([[1], [0]], np.int32)), "6x4": (6, cr.SOURCES), "6x16": (6, wide_sources())}


@pytest.mark.parametrize("name", list(cr.SIZES))
def test_matrices_equal_the_float64_restatement(hip_device, name):
    from dvmvs.hip import ops
    _, K, poses, _ = cr.scene(name)
    for sources in (cr.SOURCES, wide_sources()):
        k, p, s = up(hip_device, K, poses, sources)
        got = ops.consistency_matrices(k, p, s).cpu().numpy()
        want = cr.consistency_matrices(K, poses, sources)
        assert np.abs(want).max() > 1 and same_bits(got, want)
        skipped = np.array([[cr.skipped(int(x), r, len(K)) for x in row] for r, row in enumerate(sources)])
        assert skipped.any() and not got[skipped].any()


@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("name", ["24x32", "23x37"])        # rows of 32 floats: the 16-byte path; rows of 37: single-element accesses, ragged tail
def test_filter_equals_the_float32_restatement(hip_device, name, batch):
    n, sources = BATCHES[batch]
    depths, K, poses, _ = cr.scene(name)
    depths, K, poses = depths[:n], K[:n], poses[:n]
    kept = []
    for average in (False, True):
        for min_views in (0, 2, 5):
            kwargs = dict(average=average, min_views=min_views)
            got = filtered(hip_device, depths, K, poses, sources, **kwargs)
            assert_equals_restatement(got, depths, K, poses, sources, **kwargs)
            kept.append(int((got[0] > 0).sum()))
    valid = int(cr._valid(depths).sum())
    assert kept[0] == kept[3] == valid and kept[2] == kept[5] == 0        # min_views 0 keeps every valid pixel; 5 of at most 4 sources: none
    if n == 6:
        assert 0.6 * valid <= kept[1] == kept[4] < valid
    else:
        assert kept[1] == 0                                               # fewer than two sources


def test_other_thresholds(hip_device):
    depths, K, poses, sources = cr.scene("23x37")
    for kwargs in (dict(pixel_threshold=0.3, relative_threshold=0.002), dict(pixel_threshold=2.5, relative_threshold=0.1, min_views=1)):
        assert_equals_restatement(filtered(hip_device, depths, K, poses, sources, **kwargs), depths, K, poses, sources, **kwargs)


def test_rows_off_the_16_byte_grid_give_the_same_bits(hip_device):
    """24x32 from buffers that start one element off a 16-byte boundary: the launch takes single-element accesses, as it does for the
    37-wide scene, and writes what the aligned launch writes."""
    from dvmvs.hip import ops
    depths, K, poses, sources = cr.scene("24x32")
    d, k, p, s = up(hip_device, depths, K, poses, sources)
    aligned, count, _ = ops.depth_consistency(d, k, p, s)
    assert d.data_ptr() % 16 == 0 and aligned.data_ptr() % 16 == 0
    shifted_in = torch.empty(d.numel() + 1, dtype=torch.float32, device=hip_device)[1:].view(d.shape).copy_(d)
    backing = torch.full((d.numel() + 2,), -7.0, dtype=torch.float32, device=hip_device)
    out = backing[1:-1].view(d.shape)
    assert shifted_in.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 4 and out.is_contiguous()
    for source in (d, shifted_in):
        backing.fill_(-7.0)
        got, got_count, _ = ops.depth_consistency(source, k, p, s, out=out)
        assert got.data_ptr() == out.data_ptr() and torch.equal(got, aligned) and torch.equal(got_count, count)
        assert backing[0] == -7.0 and backing[-1] == -7.0                 # nothing written around the view
    want = cr.scene_result("24x32", "float32")
    assert same_bits(aligned.cpu().numpy(), want["depth"]) and same_bits(count.cpu().numpy(), want["count"])


def test_a_frame_filtered_alone_has_the_bits_it_has_in_the_batch(hip_device):
    depths, K, poses, _ = cr.scene("23x37")
    batch_sources = cr.SOURCES.copy()
    batch_sources[0], batch_sources[1], batch_sources[3] = [1, 3, -1, 3], [0, 3, 0, 9], [0, 1, 6, 3]        # frames 0, 1, 3 use each other only
    whole = filtered(hip_device, depths, K, poses, batch_sources)
    picked = [3, 0, 1]
    alone_sources = np.array([[1, 2, 3, 0], [2, 0, -1, 0], [1, 0, 1, 9]], np.int32)                           # the same rows, re-indexed
    alone = filtered(hip_device, depths[picked], K[picked], poses[picked], alone_sources)
    for w, a in zip(whole, alone):
        assert same_bits(np.ascontiguousarray(w[picked]), a)
    assert int((alone[0] > 0).sum()) > 0.3 * alone[0].size


def test_two_calls_give_equal_bytes(hip_device):
    depths, K, poses, sources = cr.scene("64x80")
    first = filtered(hip_device, depths, K, poses, sources)
    second = filtered(hip_device, depths, K, poses, sources)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))
    assert_equals_restatement(first, depths, K, poses, sources)


def test_invalid_depths_give_nothing_and_poison_no_neighbour(hip_device):
    depths, K, poses, sources = cr.scene("24x32")
    bad = [(0, 0), (1, 1), (2, 2)]
    assert np.isnan(depths[cr.BROKEN_VIEW, 0, 0]) and np.isinf(depths[cr.BROKEN_VIEW, 1, 1]) and depths[cr.BROKEN_VIEW, 2, 2] < 0
    got = filtered(hip_device, depths, K, poses, sources, min_views=0)
    for y, x in bad:
        assert got[0][cr.BROKEN_VIEW, y, x] == 0 and got[1][cr.BROKEN_VIEW, y, x] == 0 and not got[2][cr.BROKEN_VIEW, y, x].any()
    assert np.isfinite(got[0]).all() and np.isfinite(got[2]).all()
    # a NaN, an inf and a negative depth act on the other views exactly as a hole (0) at the same place does
    holes = depths.copy()
    for y, x in bad:
        holes[cr.BROKEN_VIEW, y, x] = 0.0
    assert all(same_bits(a, b) for a, b in zip(got, filtered(hip_device, holes, K, poses, sources, min_views=0)))


def test_filter_depths_conveniences(hip_device):
    """numpy inputs, one [3,3] K for all frames, default sources; and the fused point cloud."""
    from dvmvs.consistency import filter_depths, fused_point_cloud, nearest_sources
    depths, K, poses, _ = cr.scene("24x32")
    depth, count, points = filter_depths(depths, K[0], poses, device=hip_device, with_points=True)
    want = cr.depth_consistency(depths, K, poses, nearest_sources(6, 4))
    assert same_bits(depth.cpu().numpy(), want["depth"]) and same_bits(count.cpu().numpy(), want["count"])
    colours = np.random.default_rng(3).integers(0, 256, depths.shape + (3,)).astype(np.uint8)
    cloud = fused_point_cloud(depth, points, colours).cpu().numpy()
    kept = want["depth"] > 0
    assert cloud.shape == (int(kept.sum()), 6) and same_bits(np.ascontiguousarray(cloud[:, :3]), want["points"][kept])
    assert np.array_equal(cloud[:, 3:], colours[kept].astype(np.float32))
    assert same_bits(fused_point_cloud(depth, points).cpu().numpy(), want["points"][kept])


# ---- LiveFusion ---------------------------------------------------------------------------------------------------------------------
ANALYTIC_BOUNDS = np.array([[-2.0, 2.0], [-1.5, 1.5], [1.0, 2.5]])


def volumes(vol):
    return vol._tsdf, vol._weight, vol._color


def same_volumes(a, b):
    return all(torch.equal(x, y) for x, y in zip(volumes(a), volumes(b)))


def test_live_fusion_without_the_filter_is_unchanged(hip_device):
    from dvmvs.tsdf import LiveFusion
    depth, rgb = fuse_scene.frames()
    poses = fuse_scene.poses()
    lives = [LiveFusion(fuse_scene.BOUNDS.copy(), voxel_size=fuse_scene.VOXEL, batch=4, device=hip_device, **kwargs)
             for kwargs in ({}, {"min_consistent_views": 0})]
    for live in lives:
        for i in range(6):
            live.add(torch.from_numpy(depth[i]).to(hip_device), rgb[i], fuse_scene.K, poses[i])
    assert lives[1]._filtered is None and lives[1]._source_tables is None        # nothing allocated for the filter
    assert int((lives[0].volume._weight > 0).sum()) >= 7000 and same_volumes(lives[0].volume, lives[1].volume)


@pytest.mark.parametrize("which", ["analytic", "fuse_scene"])
def test_live_fusion_with_the_filter(hip_device, which):
    """Six frames with batch = 5: a flush of five, filtered against each other, and a last flush of ONE pending frame, which has no neighbour
    and fuses nothing.  The adds after the first run with PyTorch's synchronisation detector armed."""
    from dvmvs.consistency import filter_depths
    from dvmvs.tsdf import LiveFusion, TSDFVolume
    if which == "analytic":
        depth, Ks, poses, _ = cr.scene("24x32")
        K, bounds, voxel = Ks[0], ANALYTIC_BOUNDS, 0.05
        rgb = np.random.default_rng(4).integers(0, 256, depth.shape + (3,)).astype(np.uint8)
    else:
        depth, rgb = fuse_scene.frames()
        poses, K, bounds, voxel = fuse_scene.poses(), fuse_scene.K, fuse_scene.BOUNDS, fuse_scene.VOXEL
    live = LiveFusion(bounds.copy(), voxel_size=voxel, max_depth=2.3, batch=5, device=hip_device, min_consistent_views=2)
    on_device = up(hip_device, *depth)
    live.add(on_device[0], rgb[0], K, poses[0])
    torch.cuda.synchronize(hip_device)
    torch.cuda.set_sync_debug_mode("error")
    try:
        for i in range(1, 6):
            live.add(on_device[i], rgb[i], K, poses[i])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert live._pending == 1
    want = TSDFVolume(bounds.copy(), voxel, device=hip_device)
    kept, _, _ = filter_depths(depth[:5], K, poses[:5], n_sources=4, min_views=2, average=False, device=hip_device)
    want.integrate_frames(rgb[:5], kept, K, poses[:5], max_depth=2.3)
    assert same_volumes(live._volume, want)                   # the sixth frame is pending
    assert same_volumes(live.volume, want) and live._pending == 0 and live.frames == 6        # ... and fuses nothing
    if which == "analytic":
        unfiltered = TSDFVolume(bounds.copy(), voxel, device=hip_device)
        unfiltered.integrate_frames(rgb[:5], depth[:5], K, poses[:5], max_depth=2.3)
        seen, seen_unfiltered = int((want._weight > 0).sum()), int((unfiltered._weight > 0).sum())
        assert 0 < seen < seen_unfiltered and int((kept > 0).sum()) > 0.5 * kept.numel()


# ---- the program --------------------------------------------------------------------------------------------------------------------
def _surface_distance(points):
    """Distance of world points from the analytic scene: the plane z = 2.2 or the sphere."""
    p = points.astype(np.float64)
    return np.minimum(np.abs(p[:, 2] - cr.PLANE_Z), np.abs(np.linalg.norm(p - cr.SPHERE_CENTRE, axis=1) - cr.SPHERE_RADIUS))


def test_program_filters_and_writes_the_point_cloud(hip_device, tmp_path, capsys):
    """``python -m dvmvs.tsdf --filter_consistency --save_point_cloud`` on six 64x80 keyframes of the analytic scene (its exact depth as
    'predictions', one TRACKING LOST line); and without the flags: the one file of before, with the bytes of a fusion made here through
    the public classes."""
    from PIL import Image
    from dvmvs.consistency import filter_depths, nearest_sources
    from dvmvs.dataset_loader import PreprocessImage, load_image
    from dvmvs.tsdf import TSDFFusion, TSDFVolume, main
    depths, Ks, poses = cr.clean_scene("64x80")
    h, w = depths.shape[1:]
    voxel = 0.05
    scene_dir = tmp_path / "data" / "hololens-dataset" / "000"
    (scene_dir / "images").mkdir(parents=True)
    rng = np.random.default_rng(5)
    names = [f"{i:05d}.png" for i in range(6)]
    for name in names:
        Image.fromarray(rng.integers(0, 256, (h, w, 3)).astype(np.uint8)).save(scene_dir / "images" / name)
    np.savetxt(scene_dir / "poses.txt", poses.reshape(-1, 16).astype(np.float64))
    np.savetxt(scene_dir / "K.txt", Ks[0].astype(np.float64))
    (tmp_path / "data" / "indices").mkdir()
    lines = [f"{n} {n}" for n in names]
    (tmp_path / "data" / "indices" / "keyframe+hololens-dataset+000+nmeas+3").write_text("\n".join(lines[:3] + ["TRACKING LOST"] + lines[3:]) + "\n")
    (tmp_path / "pred").mkdir()
    system = "320_256_3_dvmvs_fusionnet_online"
    np.savez(tmp_path / "pred" / f"keyframe_hololens-dataset_{system}_predictions_000.npz", depths)
    common = ["--prediction_folder", str(tmp_path / "pred"), "--data_folder", str(tmp_path / "data"), "--voxel_size", str(voxel)]
    main(["--reconstruction_folder", str(tmp_path / "plain")] + common)
    capsys.readouterr()
    main(["--reconstruction_folder", str(tmp_path / "filtered"), "--filter_consistency", "--save_point_cloud"] + common)
    printed = capsys.readouterr().out
    assert "Consistency filter: kept" in printed

    # without the flags: the file list of before, and the bytes of the same fusion made here
    stem = f"reconstruction_voxelsize-{voxel}_maxdepth-5.0_anchor-False_{{}}_hololens-dataset_000"
    assert sorted(os.listdir(tmp_path / "plain")) == [stem.format(system) + "_complete.ply"]
    images = [load_image(str(scene_dir / "images" / n)) for n in names]
    scaled_K = PreprocessImage(K=Ks[0], old_width=w, old_height=h, new_width=w, new_height=h, distortion_crop=0,
                               perform_crop=False).get_updated_intrinsics()
    poses64 = np.fromfile(str(scene_dir / "poses.txt"), dtype=float, sep="\n ").reshape((-1, 4, 4))
    bounds = TSDFFusion.calculate_volume_bounds(list(depths), list(poses64), scaled_K) * 1.05
    volume = TSDFVolume(bounds.copy(), voxel_size=voxel, device=hip_device)
    for image, depth, pose in zip(images, depths, poses64):
        volume.integrate(image.astype(np.uint8), depth, scaled_K, pose, obs_weight=1.0)
    TSDFFusion.meshwrite(str(tmp_path / "expected.ply"), *volume.get_mesh())
    plain_bytes = open(tmp_path / "plain" / (stem.format(system) + "_complete.ply"), "rb").read()
    assert plain_bytes == open(tmp_path / "expected.ply", "rb").read() and len(plain_bytes) > 10000

    # with the flags: the +consistent mesh and the point cloud, nothing else
    mesh, cloud_file = (stem.format(system + "+consistent") + tail for tail in ("_complete.ply", "_pointcloud.ply"))
    assert sorted(os.listdir(tmp_path / "filtered")) == [mesh, cloud_file]
    with open(tmp_path / "filtered" / mesh) as f:
        header = [next(f).strip() for _ in range(3)]
    assert header[:2] == ["ply", "format ascii 1.0"] and 0 < int(header[2].split()[-1])
    text = open(tmp_path / "filtered" / cloud_file).read().split("end_header\n")
    vertices = int([line for line in text[0].splitlines() if line.startswith("element vertex")][0].split()[-1])
    cloud = np.array([row.split() for row in text[1].splitlines()], dtype=np.float64)
    sources = nearest_sources(6, 4, [0, 0, 0, 1, 1, 1])
    kept, _, points = filter_depths(depths, scaled_K, poses, sources, min_views=2, average=True, with_points=True, device=hip_device)
    kept_pixels = int((kept > 0).sum())
    valid = int((depths > 0).sum())
    print(f"point cloud: {vertices} points of {valid} valid pixels; farthest from the surface {_surface_distance(cloud[:, :3]).max():.4f} m")
    assert cloud.shape == (vertices, 6) and vertices == kept_pixels and 0.3 * valid < kept_pixels <= valid
    assert _surface_distance(cloud[:, :3]).max() <= voxel
    assert np.abs(cloud[:, :3] - points[kept > 0].cpu().numpy()).max() < 1e-6 + 1e-6        # "%f": six decimals
    assert f"kept {100.0 * kept_pixels / valid:.1f} %" in printed

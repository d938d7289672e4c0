"""GPU: csrc/mesh_raster.hip against the numpy restatement of its definition (tests/mesh_raster_reference.py) -- depth compared as int32
bit patterns, faces and overflow counts exactly -- then against the float64 reference within the derived bounds, the vertex visibility,
``dvmvs.tsdf.visible_mesh``, ``TSDFVolume.score_against(visible_from=...)`` and ``python -m dvmvs.tsdf --evaluate_3d_visible``.  The
restatement is handed the world-to-camera matrices the device used, so the comparison starts from equal inputs."""
import os

import numpy as np
import pytest
import torch

import mesh_raster_reference as R

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def on(dev, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)


def device_raster(dev, verts, faces, K, P, H, W, **kwargs):
    """(depth, face, overflow) of the device as numpy arrays, and the world-to-camera matrices it used."""
    from dvmvs.hip import ops
    from dvmvs.hip.ops import reconstruction
    tv, tf, tK, tP = on(dev, verts, faces, K, P)
    depth, face, overflow = ops.mesh_raster(tv, tf, tK, tP, H, W, return_overflow=True, **kwargs)
    assert depth.is_cuda and depth.dtype == torch.float32 and face.dtype == torch.int32 and overflow.dtype == torch.int32
    assert tuple(depth.shape) == tuple(face.shape) == (len(K), H, W) and tuple(overflow.shape) == (len(K),)
    return depth.cpu().numpy(), face.cpu().numpy(), overflow.cpu().numpy(), reconstruction.mesh_raster_cameras(tP).cpu().numpy()


def assert_bits(dev, case, near=0.05, far=float("inf"), cull_backfaces=False, **device_only):
    verts, faces, K, P, H, W = case
    depth, face, overflow, w2c = device_raster(dev, verts, faces, K, P, H, W, near=near, far=far, cull_backfaces=cull_backfaces, **device_only)
    want = R.raster_fp32(verts, faces, K, w2c, H, W, near=near, far=far, cull_backfaces=cull_backfaces)
    print(f"V {len(verts)} F {len(faces)} N {len(K)} {H}x{W}: {100 * (face >= 0).mean():.1f} % of the pixels hit, overflow {overflow.tolist()}")
    assert np.array_equal(face, want[1])
    assert np.array_equal(bits(depth), bits(want[0]))
    assert np.array_equal(overflow, want[2])
    return depth, face, overflow


def test_world_to_camera_matrices(hip_device):
    """The device's float64 inverse, rounded once, against numpy's: equal but for the last bit of an entry."""
    from dvmvs.hip.ops import reconstruction
    _, poses = R.views(5)
    poses = np.concatenate([poses, R.room_mesh()[3]])
    got = reconstruction.mesh_raster_cameras(torch.from_numpy(poses).to(hip_device)).cpu().numpy()
    want = R.world_to_camera(poses)
    assert got.shape == (len(poses), 3, 4) and got.dtype == np.float32
    assert np.abs(got.astype(np.float64) - want).max() <= 2.0 ** -23 * np.abs(want).max()
    assert (got != want).mean() < 0.05


# ---- bit equality with the restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fan", "quad", "floor", "behind", "duplicates", "overflow"])
def test_hand_cases(hip_device, name):
    depth, face, overflow = assert_bits(hip_device, R.hand_cases()[name])
    if name == "fan":
        for f, expected in R.FAN_PIXELS.items():
            vs, us = np.nonzero(face[0] == f)
            assert sorted(zip(us.tolist(), vs.tolist())) == sorted(expected)
    if name == "behind":
        assert np.all(depth == 0) and np.all(face == -1)
    if name == "overflow":
        assert overflow.tolist() == [1] and set(np.unique(face)) == {-1, 1}
    if name == "duplicates":
        assert set(np.unique(face)) == {-1, 0}


@pytest.mark.parametrize("name", ["grid", "soup"])
def test_random_meshes_one_view(hip_device, name):
    assert_bits(hip_device, R.random_case(name))


@pytest.mark.parametrize("size", [(48, 64), (33, 47), (1, 1)])
@pytest.mark.parametrize("name", ["grid", "soup"])
def test_three_views_with_their_own_intrinsics(hip_device, name, size):
    verts, faces = R.random_case(name)[:2]
    K, P = R.views(3)
    assert_bits(hip_device, (verts, faces, K, P) + size)


def whole_image_triangle():
    K, P = R.exact_camera()
    verts, faces = R.pixel_triangle([[-40, -30], [200, -20], [-30, 160]], [2.0, 4.0, 3.0])
    return verts, faces, K, P


@pytest.mark.parametrize("size", [(48, 64), (33, 47), (1, 1)])
def test_one_triangle_over_the_whole_image_takes_the_list(hip_device, size):
    """F = 1; its box is the image, cut into every 16x16 tile of the grid (ragged at 33x47)."""
    from dvmvs.hip.ops import reconstruction
    depth, face, _ = assert_bits(hip_device, whole_image_triangle() + size)
    assert np.all(face == 0) and np.all(depth > 0)
    if size != (1, 1):
        assert size[0] * size[1] > reconstruction.MESH_RASTER_LARGE_BOX
    alone = assert_bits(hip_device, whole_image_triangle() + size, large_box=10 ** 9)          # the same by the thread of its face
    assert np.array_equal(bits(alone[0]), bits(depth))


@pytest.mark.parametrize("large_box", [1, 10 ** 9])
def test_every_face_on_one_path(hip_device, large_box):
    """The grid mesh with every piece on the list (large_box = 1: every box has more pixels, or none) and with none."""
    verts, faces = R.random_case("grid")[:2]
    K, P = R.views(3)
    assert_bits(hip_device, (verts, faces, K, P, 48, 64), large_box=large_box)


def test_boxes_around_the_threshold(hip_device):
    """Triangles whose pixel boxes hold one pixel fewer than, exactly, and more than ``MESH_RASTER_LARGE_BOX``, overlapping, among small ones."""
    from dvmvs.hip.ops import reconstruction
    side = int(np.sqrt(reconstruction.MESH_RASTER_LARGE_BOX))
    assert side * side == reconstruction.MESH_RASTER_LARGE_BOX and side + 1 < 40
    K, P = R.exact_camera()
    meshes = []
    for i, (w, h) in enumerate(((side, side), (side, side + 1), (side - 1, side + 1), (side + 1, side + 1), (side, side))):
        x0, y0 = 3.5 + 7 * i, 2.5 + 4 * i                  # the box holds the pixels x0 + 0.5 .. x0 + w - 0.5: w columns
        meshes.append(R.pixel_triangle([[x0, y0], [x0 + w - 0.1, y0], [x0, y0 + h - 0.1]], [2.0 + 0.1 * i, 3.0, 2.5])[0])
    soup = R.soup_mesh(seed=4, count=40)[0]
    verts = np.concatenate(meshes + [soup])
    faces = np.arange(len(verts), dtype=np.int32).reshape(-1, 3)
    assert_bits(hip_device, (verts, faces, K, P, 48, 64))


def test_camera_inside_a_closed_box(hip_device):
    """Every pixel is hit; each of the 12 faces crosses the near plane or lies behind the camera in some view."""
    verts, faces = R.box_mesh()
    eye = (0.1, 0.05, -0.2)
    P = np.stack([R.look_at(eye, t) for t in ((0.3, 0.1, 1.0), (1.0, -0.4, 0.2), (-0.5, 1.0, -0.3), (-1.0, -1.0, -1.0))])
    P[3] = P[3] @ np.array([[0.8, -0.6, 0, 0], [0.6, 0.8, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)       # rolled about its axis
    K = np.stack([R.intrinsics(40.0 + 10 * i, 31.5, 23.5) for i in range(4)])
    depth, face, overflow = assert_bits(hip_device, (verts, faces, K, P, 48, 64))
    assert np.all(face >= 0) and np.all(depth >= 0.05) and overflow.tolist() == [0, 0, 0, 0]
    assert_bits(hip_device, (verts, faces, K, P, 48, 64), cull_backfaces=True)
    assert_bits(hip_device, (verts, faces[:, ::-1].copy(), K, P, 48, 64), cull_backfaces=True, far=1.2)


def test_faces_with_bad_indices_and_an_empty_mesh(hip_device):
    from dvmvs.hip import ops
    verts, faces, K, P, H, W = R.hand_cases()["fan"]
    bad = np.concatenate([np.array([[0, 1, 99], [-1, 2, 3]], dtype=np.int32), faces])
    assert_bits(hip_device, (verts, bad, K, P, H, W))
    tv, tf, tK, tP = on(hip_device, verts, faces, K, P)
    depth, face = ops.mesh_raster(tv, tf[:0], tK, tP, H, W)
    assert float(depth.abs().max()) == 0 and int(face.max()) == -1


def test_workspace_of_the_caller_is_reused_across_sizes(hip_device):
    """Garbage in the buffer, then a large call, then a small one in the same buffer: each equals the call with the per-device workspace."""
    from dvmvs.hip import ops
    from dvmvs.hip.ops import reconstruction
    big = R.random_case("grid")[:2] + R.views(3) + (48, 64)
    small = whole_image_triangle() + (33, 47)
    nbytes = max(reconstruction.mesh_raster_workspace_bytes(len(c[2]), len(c[1]), c[4], c[5]) for c in (big, small))
    workspace = torch.randint(-2 ** 62, 2 ** 62, (nbytes // 8 + 1,), dtype=torch.int64, device=hip_device)
    for case in (big, small, big):
        fresh = assert_bits(hip_device, case)
        reused = assert_bits(hip_device, case, workspace=workspace)
        assert np.array_equal(bits(fresh[0]), bits(reused[0])) and np.array_equal(fresh[1], reused[1])
    with pytest.raises(ValueError, match="workspace"):
        ops.mesh_raster(*on(hip_device, *big[:4]), 48, 64, workspace=workspace[:16])


def test_result_does_not_depend_on_the_order_of_the_faces(hip_device):
    verts, faces = R.random_case("soup")[:2]
    grid_verts, grid_faces = R.random_case("grid")[:2]
    verts, faces = np.concatenate([verts, grid_verts]), np.concatenate([faces, grid_faces + len(verts)])
    K, P = R.views(3)
    order = np.random.default_rng(5).permutation(len(faces))
    a = device_raster(hip_device, verts, faces, K, P, 48, 64)
    b = device_raster(hip_device, verts, faces[order], K, P, 48, 64)
    assert np.array_equal(bits(a[0]), bits(b[0]))
    assert np.array_equal(a[1], np.where(b[1] >= 0, order[np.maximum(b[1], 0)], -1))


# ---- geometry against float64 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grid", "soup"])
def test_device_against_float64(hip_device, name):
    verts, faces, K, P, H, W = R.random_case(name)
    depth, face, _, _ = device_raster(hip_device, verts, faces, K, P, H, W)
    excluded = R.compare_with_f64(depth, face, R.random_reference(name))
    print(f"{name}: {100 * excluded:.2f} % of the pixels excluded")
    assert excluded <= R.MAX_EXCLUDED


# ---- visibility -------------------------------------------------------------------------------------------------------
def device_count(dev, verts, depth, K, P, **kwargs):
    from dvmvs.hip import ops
    count = ops.mesh_visibility(*on(dev, verts, depth, K, P), **kwargs)
    assert count.dtype == torch.int32 and tuple(count.shape) == (len(verts),)
    return count.cpu().numpy()


@pytest.mark.parametrize("name", ["grid", "soup"])
def test_visibility_equals_the_restatement(hip_device, name):
    verts, faces = R.random_case(name)[:2]
    K, P = R.views(3)
    depth, _, _, w2c = device_raster(hip_device, verts, faces, K, P, 33, 47)
    for kwargs in ({}, {"relative": 0.0, "absolute": 0.02}, {"near": 1.5}):
        want = R.visibility_fp32(verts, depth, K, w2c, **kwargs)
        got = device_count(hip_device, verts, depth, K, P, **kwargs)
        print(f"{name} {kwargs}: seen by 0..3 views: {np.bincount(want, minlength=4).tolist()}")
        assert np.array_equal(got, want)
    holes = depth.copy()
    holes[:, ::3, ::2] = 0
    holes[0, 5, 7] = np.nan
    assert np.array_equal(device_count(hip_device, verts, holes, K, P), R.visibility_fp32(verts, holes, K, w2c))


def test_visible_mesh_on_two_walls(hip_device):
    from dvmvs.tsdf import visible_mesh
    verts, faces, K, P, H, W, n_near = R.two_walls()
    depth, _, _, w2c = device_raster(hip_device, verts, faces, K, P, H, W)
    seen = R.visibility_fp32(verts, depth, K, w2c)
    assert np.array_equal(device_count(hip_device, verts, depth, K, P), seen)
    assert np.all(seen[:n_near] == 1) and (seen[n_near:] == 0).sum() >= 9
    want = R.kept_faces(faces, seen)
    kept_verts, kept = visible_mesh(verts, faces, K[0], P[0], H, W)
    assert kept.is_cuda and kept.dtype == torch.int32 and np.array_equal(kept_verts.cpu().numpy(), verts)
    assert 0 < len(want) < len(faces) and np.array_equal(kept.cpu().numpy(), want)
    twice = visible_mesh(verts, faces, np.repeat(K, 2, axis=0), np.repeat(P, 2, axis=0), H, W, min_views=2)[1]
    assert np.array_equal(twice.cpu().numpy(), want)
    assert len(visible_mesh(verts, faces, K, P, H, W, min_views=2)[1]) == 0


def test_visible_mesh_in_chunks(hip_device, monkeypatch):
    from dvmvs import tsdf
    verts, faces, K, P, H, W = R.room_mesh()
    whole = tsdf.visible_mesh(verts, faces, K, P, H, W, min_views=2)[1]
    from dvmvs.tsdf import mesh_views
    monkeypatch.setattr(mesh_views, "VISIBLE_MESH_CHUNK", 3)          # the module that owns it: visible_mesh reads it there
    assert torch.equal(tsdf.visible_mesh(verts, faces, K, P, H, W, min_views=2)[1], whole)
    assert 0 < len(whole) < len(faces)


def test_render_mesh(hip_device):
    from dvmvs.tsdf import render_mesh
    verts, faces, K, P, H, W = R.hand_cases()["overflow"]
    with pytest.warns(RuntimeWarning, match="left out"):
        depth, face = render_mesh(verts, faces, K[0], P[0], H, W)
    want = device_raster(hip_device, verts, faces, K, P, H, W)
    assert np.array_equal(bits(depth.cpu().numpy()), bits(want[0])) and np.array_equal(face.cpu().numpy(), want[1])


# ---- scoring against what the cameras saw -----------------------------------------------------------------------------
ROOM_VOXEL = 2.5 / 64          # exact in binary: [-1.25, 1.25]^3 is 64 voxels a side


@pytest.fixture(scope="module")
def room(hip_device):
    """The room, its depth maps from the eight views (rasterised: synthetic sensor depth), and a 64^3 volume fused from them."""
    from dvmvs.hip import ops
    from dvmvs.tsdf import TSDFVolume
    verts, faces, K, P, H, W = R.room_mesh()
    depth, _ = ops.mesh_raster(*on(hip_device, verts, faces, K, P), H, W)
    volume = TSDFVolume(np.array([[-1.25, 1.25]] * 3), ROOM_VOXEL, device=hip_device)
    assert tuple(volume.vol_dim) == (64, 64, 64)
    volume.integrate_frames(torch.zeros((len(P), H, W, 3), dtype=torch.uint8, device=hip_device), depth, K, P)
    return volume, (verts, faces, K, P, H, W), depth


def test_score_against_visible_part(hip_device, room):
    from dvmvs import errors
    from dvmvs.tsdf import visible_mesh
    volume, (verts, faces, K, P, H, W), _ = room
    density = 2000.0
    full = volume.score_against((verts, faces), 0.05, sample_density=density).cpu().numpy()
    row, sizes, kept = volume.score_against((verts, faces), 0.05, return_sizes=True, sample_density=density, visible_from=(K, P, H, W))
    row = row.cpu().numpy()
    print(f"full room {full}, visible part {row}: {kept[0]} of {kept[1]} faces, {sizes} points")
    assert kept[1] == len(faces) and 0 < kept[0] < len(faces) // 2                   # two of six walls at most
    assert full[4] < row[4]                                                          # recall
    kept_verts, kept_faces = visible_mesh(verts, faces, K, P, H, W)
    assert len(kept_faces) == kept[0]
    pred_verts, pred_faces = volume.mesh_tensors()
    by_hand = errors.compute_reconstruction_errors_device(pred_verts, kept_verts, 0.05, pred_faces=pred_faces, gt_faces=kept_faces,
                                                          sample_density=density)
    assert np.array_equal(bits(by_hand.cpu().numpy()), bits(row))
    # a TSDFVolume as the reference goes through its mesh; a bare point set is refused
    own = volume.score_against(volume, 0.05, sample_density=density, visible_from=(K, P, H, W, 2)).cpu().numpy()
    assert own[4] == 1                                                               # every kept face is part of the prediction
    with pytest.raises(ValueError, match="point set"):
        volume.score_against(verts, 0.05, sample_density=density, visible_from=(K, P, H, W))
    with pytest.raises(ValueError, match="sample_density"):
        volume.score_against((verts, faces), 0.05, visible_from=(K, P, H, W))


def test_mesh_and_volume_renderers_agree(hip_device, room):
    """Two independent renderers of one surface: the rasterised marching-cubes mesh and the ray-cast volume, within a voxel nearly everywhere."""
    from dvmvs.tsdf import render_mesh
    volume, (_, _, K, P, H, W), _ = room
    cast = volume.render(K, P, H, W, normals=False, colour=False)[0]
    drawn = render_mesh(*volume.mesh_tensors(), K, P, H, W)[0]
    both = (cast > 0) & (drawn > 0)
    difference = (cast - drawn).abs()[both] / ROOM_VOXEL
    print(f"{100 * float(both.float().mean()):.1f} % of the pixels hit by both; median |difference| {float(difference.median()):.4f} voxels")
    assert float(both.float().mean()) > 0.5 and float(difference.median()) < 0.5


# ---- the program ------------------------------------------------------------------------------------------------------
def test_program_scores_against_the_visible_part(hip_device, room, tmp_path):
    from PIL import Image
    from dvmvs.tsdf import TSDFFusion, main
    _, (verts, faces, K, P, H, W), depth = room
    scene_dir = tmp_path / "data" / "hololens-dataset" / "000"
    (scene_dir / "images").mkdir(parents=True)
    names = ["%05d.png" % i for i in range(len(P))]
    for name in names:
        Image.fromarray(np.full((H, W, 3), 128, dtype=np.uint8)).save(scene_dir / "images" / name)
    np.savetxt(scene_dir / "poses.txt", P.astype(np.float64).reshape(-1, 16))
    np.savetxt(scene_dir / "K.txt", K[0].astype(np.float64))
    (tmp_path / "data" / "indices").mkdir()
    (tmp_path / "data" / "indices" / "keyframe+hololens-dataset+000+nmeas+3").write_text("".join(f"{n} {names[0]}\n" for n in names))
    (tmp_path / "pred").mkdir()
    np.savez(tmp_path / "pred" / "keyframe_hololens-dataset_320_256_3_dvmvs_fusionnet_online_predictions_000.npz", depth.cpu().numpy())
    mesh_path = str(tmp_path / "room.ply")
    TSDFFusion.meshwrite(mesh_path, verts, faces, np.zeros_like(verts), np.zeros((len(verts), 3), np.uint8))
    common = ["--prediction_folder", str(tmp_path / "pred"), "--data_folder", str(tmp_path / "data"), "--voxel_size", "0.05", "--evaluate_3d",
              "--groundtruth_mesh", mesh_path, "--evaluate_3d_density", "1000"]
    saved = {}
    for tag, flags in (("full", []), ("visible", ["--evaluate_3d_visible"])):
        out = tmp_path / tag
        main(["--reconstruction_folder", str(out)] + common + flags)
        errors_file, = [w for w in os.listdir(out) if w.endswith("_errors3d.npz")]
        saved[tag] = np.load(out / errors_file)
    assert "visible_faces" not in saved["full"].files and "total_faces" not in saved["full"].files
    visible, total = int(saved["visible"]["visible_faces"]), int(saved["visible"]["total_faces"])
    print(f"{visible} of {total} faces; recall {saved['full']['arr_0'][4]:.3f} -> {saved['visible']['arr_0'][4]:.3f}")
    assert total == len(faces) and 0 < visible < total
    assert saved["full"]["arr_0"][4] < saved["visible"]["arr_0"][4]

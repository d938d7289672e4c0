"""GPU: the point-to-plane registration (csrc/registration.hip, dvmvs.hip.registration.icp_plane) against its host definition
(dvmvs.errors.register_points_plane, which tests/test_registration_plane_reference.py pins on the CPU) -- one iteration, the solve and the
whole loop bit for bit -- and the surface built on it: ``compute_reconstruction_errors_device(align_plane=True)``,
``TSDFVolume.score_against(align_plane=True)`` and the program's ``--evaluate_3d_align_plane``.  A host answer is computed once per case."""
import os

import numpy as np
import pytest
import torch

import registration_plane_reference as pr
import registration_reference as rr
import tsdf_fuse_scene as scene
from dvmvs import errors

pytestmark = pytest.mark.gpu

RECORDED = ("fitness", "rmse", "rmse_point")


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def off_boundary(dev, cloud):
    """``cloud`` as a device tensor whose storage starts 4 bytes past a 16-byte boundary."""
    flat = torch.empty(cloud.size + 1, dtype=torch.float32, device=dev)
    view = flat[1:].view(-1, 3)
    view.copy_(torch.from_numpy(np.ascontiguousarray(cloud)))
    assert view.data_ptr() % 16 == 4
    return view


def on_side_stream(dev, call):
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        result = call()
    side.synchronize()
    torch.cuda.current_stream(dev).wait_stream(side)
    return result


def up(dev, *arrays):
    return [torch.from_numpy(np.array(a)).to(dev) for a in arrays]


def assert_record(got_T, got, want_T, want, label):
    """Everything the state block records against the host definition, bit for bit."""
    got = {k: v.cpu().numpy() for k, v in got.items()}
    k = want["iterations"]
    assert int(got["iterations"]) == k and int(got["status"]) == want["status"], (label, got["iterations"], got["status"], want["status"])
    assert np.array_equal(got["inliers"][:k], want["inliers"]), (label, got["inliers"][:k], want["inliers"])
    for key in RECORDED:
        assert bits(got[key][:k]) == bits(want[key]), (label, key, got[key][:k], want[key])
    assert got["moments"].shape == (30,) and bits(got["moments"]) == bits(want["moments"]), (label, got["moments"] - want["moments"])
    difference = np.abs(got_T.cpu().numpy() - want_T).max()
    assert bits(got_T.cpu().numpy()) == bits(want_T), f"{label}: T differs by {difference:.3e}"


# ---- one iteration ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 1024, 1025, 4099, 66561])
def test_one_iteration(hip_device, N):
    """One iteration from a T_0 that moves the points, against 500 targets of which a fifth have no normal, with a distance that trims
    about half of the pairs (and one that trims none); the source starts 4 bytes off a 16-byte boundary; the call runs on a side stream.
    66 561 points are 66 block sums: the second round of the lane reduction."""
    from dvmvs.hip import registration
    source, target, normals, median = pr.one_iteration_case(N)
    t_dev, n_dev = up(hip_device, target, normals)
    s_dev = off_boundary(hip_device, source)
    for label, max_distance in (("half", median), ("none", float("inf"))):
        want_T, want = errors.register_points_plane(source, target, normals, max_distance, init=pr.START, max_iterations=1)
        assert want["inliers"][0] <= N and (N < 100 or 0 < want["inliers"][0] < N)
        T, info = on_side_stream(hip_device, lambda: registration.icp_plane(s_dev, t_dev, n_dev, max_distance, init=pr.START, max_iterations=1))
        assert T.dtype == torch.float64 and tuple(T.shape) == (4, 4) and T.is_cuda and all(v.is_cuda for v in info.values())
        assert_record(T, info, want_T, want, f"N={N} trim {label}")


# ---- the solve -------------------------------------------------------------------------------------------------------------------------
def solve_cases():
    """(name, source, target, normals, max_distance, status after one iteration): clouds made so that the single partial row of moments is
    the wanted one -- a single plane (a pivot at rounding level), five pairs, a rotation of 25 degrees (far from the small-angle regime
    the step is linearised in), and a source that already lies on its targets (b = 0: the step is the identity)."""
    corner, normals = pr.squares(600, 41)
    plane, plane_normals = pr.squares(600, 42, which=(1,))
    turn = rr.rigid([0.2, 1.0, -0.4], 25.0, [0.03, -0.02, 0.01])
    centre = corner.astype(np.float64).mean(axis=0)
    turn[:3, 3] += centre - turn[:3, :3] @ centre                                # about the cloud's centre: every point keeps a nearby target
    turned = rr.transform32(corner[:300], turn)
    return [("degenerate", pr.displaced(plane[:300]), plane, plane_normals, 0.1, pr.DEGENERATE),
            ("five", pr.displaced(corner[:5]), corner, normals, 0.1, pr.TOO_FEW),
            ("six", pr.displaced(corner[:6]), corner, normals, 0.1, None),
            ("large_rotation", turned, corner, normals, float("inf"), pr.LIMIT),
            ("identity", corner[::2].copy(), corner, normals, 0.1, pr.LIMIT)]


@pytest.mark.parametrize("case", solve_cases(), ids=lambda c: c[0])
def test_solve_on_the_device(hip_device, case):
    """T after ONE iteration: the LDL^T, the degeneracy test, the quaternion and the composition on the device against the host's."""
    from dvmvs.hip import registration
    name, source, target, normals, max_distance, status = case
    want_T, want = errors.register_points_plane(source, target, normals, max_distance, max_iterations=1)
    assert status is None or want["status"] == status, (name, want["status"])
    if name == "identity":
        assert np.array_equal(want_T, np.eye(4)) and want["rmse"][0] == 0.0
    if name == "large_rotation":
        assert np.degrees(np.arccos((np.trace(want_T[:3, :3]) - 1.0) / 2.0)) > 20.0
    T, info = registration.icp_plane(*up(hip_device, source, target, normals), max_distance, max_iterations=1)
    print(f"{name}: status {int(info['status'])}, |T - host| {np.abs(T.cpu().numpy() - want_T).max():.3e}")
    assert_record(T, info, want_T, want, name)


# ---- the whole loop --------------------------------------------------------------------------------------------------------------------
def test_whole_loop(hip_device):
    from dvmvs.hip import ops, registration
    source, target, normals = pr.corner_case(1200, 1500)
    want_T, want = pr.corner_result(1200, 1500)
    assert want["status"] == pr.CONVERGED and want["iterations"] <= 10
    s, t, n = up(hip_device, source, target, normals)
    T, info = registration.icp_plane(s, t, n, 0.1)
    print(f"{int(info['iterations'])} iterations, rmse {info['rmse'][:int(info['iterations'])].cpu().numpy()}, "
          f"|T - truth| {np.abs(T.cpu().numpy() - pr.MOTION).max():.2e}")
    assert_record(T, info, want_T, want, "corner")
    longer, info60 = registration.icp_plane(s, t, n, 0.1, max_iterations=60)          # the launches after convergence do nothing
    assert torch.equal(longer, T) and int(info60["iterations"]) == want["iterations"] and int(info60["status"]) == pr.CONVERGED
    side_T, side = on_side_stream(hip_device, lambda: errors.register_points_plane_device(s, t, n, 0.1, grid=ops.nearest_build(t)))
    assert_record(side_T, side, want_T, want, "corner, side stream, the caller's grid")
    views = [off_boundary(hip_device, np.array(a)) for a in (source, target, normals)]
    view_T, view = registration.icp_plane(*views, 0.1)
    assert_record(view_T, view, want_T, want, "corner, unaligned views")
    flipped_T, flipped = registration.icp_plane(s, t, -n, 0.1)
    assert_record(flipped_T, flipped, want_T, want, "corner, normals flipped")
    short_T, short = errors.register_points_plane(source, target, normals, 0.1, max_iterations=2)
    got_T, got = registration.icp_plane(s, t, n, 0.1, max_iterations=2)
    assert short["status"] == pr.LIMIT
    assert_record(got_T, got, short_T, short, "corner, 2 iterations")


def test_nothing_is_read_by_the_call(hip_device):
    """With torch's synchronisation check set to raise, a registration, the transform and the selection of the last recorded iteration
    go through: they only enqueue."""
    from dvmvs.hip import registration
    s, t, n = up(hip_device, *pr.corner_case(1200, 1500))
    registration.icp_plane(s, t, n, 0.1)                                          # the per-device workspaces exist from here on
    torch.cuda.synchronize(hip_device)
    torch.cuda.set_sync_debug_mode("error")
    try:
        T, info = registration.icp_plane(s, t, n, 0.1)
        moved = registration.transform_points(s, T)
        last = (info["iterations"] - 1).clamp(min=0).reshape(1)
        packed = torch.cat([T.reshape(-1), info["status"].double().reshape(1), info["rmse"].index_select(0, last),
                            info["rmse_point"].index_select(0, last)])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert moved.shape == s.shape and packed.shape == (19,) and int(packed[16]) == pr.CONVERGED


def test_argument_checks(hip_device):
    from dvmvs.hip import registration
    cloud = torch.zeros((8, 3), device=hip_device)
    for bad in (dict(max_distance=0.0), dict(max_distance=-1.0), dict(max_distance=float("nan")), dict(tolerance=-1.0),
                dict(tolerance=float("nan")), dict(max_iterations=0), dict(max_iterations=1025), dict(init=np.eye(3)),
                dict(init=np.full((4, 4), np.inf)), dict(init=torch.eye(4, device=hip_device)),
                dict(grid=torch.zeros(16, dtype=torch.uint8, device=hip_device))):
        with pytest.raises(ValueError):
            registration.icp_plane(cloud, cloud, cloud, **{"max_distance": 0.1, **bad})
    for source, target, normals in ((cloud[:0], cloud, cloud), (cloud, cloud[:0], cloud[:0]), (cloud.double(), cloud, cloud),
                                    (cloud, cloud.reshape(-1), cloud), (cloud, cloud, cloud[:7]), (cloud, cloud, cloud.double()),
                                    (cloud, cloud, cloud.reshape(-1))):
        with pytest.raises(ValueError):
            registration.icp_plane(source, target, normals, 0.1)
    with pytest.raises(RuntimeError):
        registration.icp_plane(cloud, cloud, cloud.cpu(), 0.1)                     # normals on another device: there is no CPU path
    state = registration.icp_plane_workspace(hip_device, 1000, 30)
    assert state.dtype == torch.float64 and state.is_cuda and state.numel() * 8 == 1536 + 12032 + 2 * 4096 + 256
    with pytest.raises(ValueError):
        registration.icp_plane_workspace(hip_device, 1000, 1025)
    for bad in (dict(align_plane=True), dict(align_plane=True, align_distance=0.1, align_scale=True), dict(gt_normals=cloud),
                dict(align_plane=True, align_distance=0.1, gt_normals=cloud, voxel=0.1), dict(align_normal_neighbours=10)):
        with pytest.raises(ValueError):
            errors.compute_reconstruction_errors_device(cloud, cloud, **bad)


# ---- the aligned metrics ---------------------------------------------------------------------------------------------------------------
OFFSET = rr.rigid([0.4, 1.0, -0.3], 1.0, np.array([0.012, -0.01, 0.0125]))      # 1 degree and 2 cm, as tests/test_registration_gpu.py


def fused(dev, frame_ids):
    from dvmvs.tsdf import TSDFVolume
    depth, rgb = scene.frames()
    poses = scene.poses()
    vol = TSDFVolume(scene.BOUNDS.copy(), scene.VOXEL, device=dev)
    vol.integrate_frames(rgb[frame_ids], depth[frame_ids], scene.K, poses[frame_ids])
    return vol


def displaced_volume(vol, motion):
    """A volume whose extracted mesh is ``vol``'s moved by ``motion``, vertices and normals: a reference in a frame of its own that is
    still a ``TSDFVolume``, so that ``score_against`` takes its marching-cubes normals."""
    from dvmvs.tsdf import TSDFVolume

    class Displaced(TSDFVolume):
        def __init__(self):
            self.__dict__.update(vol.__dict__)

        def _extract(self, color, clean):
            verts, faces, normals, colors = vol._extract(color, clean)
            R = torch.from_numpy(motion[:3, :3]).to(verts.device)
            shift = torch.from_numpy(motion[:3, 3]).to(verts.device)
            return (verts.double() @ R.T + shift).float(), faces, (normals.double() @ R.T).float(), colors

    return Displaced()


def test_score_against_with_plane_alignment(hip_device):
    """A small fused volume against its own surface moved by the inverse of OFFSET.  Vertex mode takes the reference volume's
    marching-cubes normals, sampled mode estimates them; both recover the offset, and the rows are those of the host function on the
    downloaded arrays, bit for bit."""
    away = np.linalg.inv(OFFSET)
    vol = fused(hip_device, [0, 1])
    reference = displaced_volume(vol, away)
    verts, faces = (a.cpu().numpy() for a in vol.mesh_tensors())
    ref_verts, ref_faces, ref_normals = (a.cpu().numpy() for a in reference._extract(False, None)[:3])
    plain = vol.score_against(reference, threshold=0.01).cpu().numpy()
    assert plain[3] < 0.5
    # vertex mode: the marching-cubes normals
    row, sizes, T = vol.score_against(reference, threshold=0.01, return_sizes=True, align_distance=0.1, align_plane=True, return_transform=True)
    assert T.is_cuda and T.dtype == torch.float64 and tuple(T.shape) == (4, 4) and sizes == (len(verts), len(verts))
    row, T = row.cpu().numpy(), T.cpu().numpy()
    print(f"vertices ({len(verts)}): unaligned {plain}, aligned {row}, |T - inverse motion| {np.abs(T - away).max():.2e}")
    want, want_T = errors.compute_reconstruction_errors(verts, ref_verts, 0.01, align_distance=0.1, align_plane=True, gt_normals=ref_normals,
                                                        return_transform=True)
    assert bits(row) == bits(want), (row, want)
    assert bits(T) == bits(want_T)
    assert row[3] == 1.0 and row[0] < 1e-4
    assert np.abs(T - away).max() < 1e-4
    dev_row = errors.compute_reconstruction_errors_device(*up(hip_device, verts, ref_verts), 0.01, align_distance=0.1, align_plane=True,
                                                          gt_normals=torch.from_numpy(ref_normals).to(hip_device))
    assert bits(dev_row.cpu().numpy()) == bits(row)
    # sampled mode: a mesh reference, normals estimated from its samples
    density = 400.0                                                              # about 4 000 samples: the host side stays within a second
    row_s, sizes_s, T_s = vol.score_against((ref_verts, ref_faces), threshold=0.01, return_sizes=True, sample_density=density, align_distance=0.1,
                                            align_plane=True, align_normal_neighbours=12, return_transform=True)
    row_s, T_s = row_s.cpu().numpy(), T_s.cpu().numpy()
    print(f"samples {sizes_s}: aligned {row_s}, |T - inverse motion| {np.abs(T_s - away).max():.2e}")
    want_s, want_T_s = errors.compute_reconstruction_errors(verts, ref_verts, 0.01, pred_faces=faces, gt_faces=ref_faces, sample_density=density,
                                                            align_distance=0.1, align_plane=True, align_normal_neighbours=12,
                                                            return_transform=True)
    assert bits(row_s) == bits(want_s), (row_s, want_s)
    assert bits(T_s) == bits(want_T_s)
    assert row_s[3] == 1.0 and np.abs(T_s - away).max() < 1e-4
    # without the keyword nothing changes: the point-to-point registration, and no registration
    assert bits(vol.score_against(reference, threshold=0.01, align_plane=False).cpu().numpy()) == bits(plain)
    point = vol.score_against(ref_verts, threshold=0.01, align_distance=0.1)
    assert bits(point.cpu().numpy()) == bits(vol.score_against(ref_verts, threshold=0.01, align_distance=0.1, align_plane=False).cpu().numpy())
    for bad in (dict(align_plane=True), dict(align_plane=True, align_distance=0.1, align_scale=True), dict(align_normal_neighbours=10)):
        with pytest.raises(ValueError):
            vol.score_against(reference, **bad)


# ---- the program -------------------------------------------------------------------------------------------------------------------------
def test_program_aligns_point_to_plane(hip_device, golden_dir, tmp_path):
    """``python -m dvmvs.tsdf --evaluate_3d --evaluate_3d_align 0.1 --evaluate_3d_align_plane`` on the two keyframes of the sample scene:
    the transform, the status and its name; without the new flag the files and their keys are what they were."""
    from PIL import Image
    from dvmvs.dataset_loader import load_depth_png, resize_nearest
    from dvmvs.tsdf import main
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

    def run(tag, flags):
        out = tmp_path / tag
        main(["--reconstruction_folder", str(out), "--prediction_folder", str(tmp_path / "pred"), "--data_folder", str(tmp_path / "data"),
              "--voxel_size", "0.05", "--evaluate_3d", "--threshold_3d", "0.1"] + flags)
        return {w: open(out / w, "rb").read() for w in sorted(os.listdir(out))}

    plain, point = run("plain", []), run("point", ["--evaluate_3d_align", "0.1"])
    plane = run("plane", ["--evaluate_3d_align", "0.1", "--evaluate_3d_align_plane", "--evaluate_3d_align_neighbours", "12",
                          "--evaluate_3d_align_normal_distance", "0.5"])
    mesh_file, = [w for w in plain if w.endswith("_complete.ply")]
    errors_file, = [w for w in plain if w.endswith("_errors3d.npz")]
    assert len(plain) == 2 and set(point) == set(plain) == set(plane) and point[mesh_file] == plain[mesh_file] == plane[mesh_file]
    saved, old, scored = (np.load(tmp_path / tag / errors_file) for tag in ("plain", "point", "plane"))
    assert sorted(saved.files) == ["arr_0", "counts", "names", "threshold"]
    aligned_keys = ["transform", "align_iterations", "align_status", "align_fitness", "align_rmse"]
    assert sorted(old.files) == sorted(saved.files + aligned_keys)
    assert sorted(scored.files) == sorted(saved.files + aligned_keys + ["align_status_name", "align_rmse_point"])
    T = scored["transform"]
    print(f"plane run: row {scored['arr_0']} (point {old['arr_0']}, plain {saved['arr_0']}), {scored['align_iterations']} iterations "
          f"(point {old['align_iterations']}), status {scored['align_status_name']}, rmse {scored['align_rmse']} / {scored['align_rmse_point']}")
    assert T.dtype == np.float64 and T.shape == (4, 4) and np.isfinite(T).all() and T[3].tolist() == [0, 0, 0, 1]
    assert abs(np.linalg.det(T[:3, :3]) - 1.0) < 1e-9
    assert 1 <= scored["align_iterations"] <= 30 and 1 <= scored["align_status"] <= 4
    assert str(scored["align_status_name"]) == errors.REGISTRATION_PLANE_STATUS[int(scored["align_status"])]
    # (|(p - q) . n| <= |p - q| |n|, and an estimated normal is of unit length to float32 rounding)
    assert 0.0 < scored["align_fitness"] <= 1.0 and 0.0 <= scored["align_rmse"] <= scored["align_rmse_point"] * (1.0 + 1e-6) <= 0.1 * (1.0 + 1e-6)
    assert scored["arr_0"].dtype == np.float32 and np.array_equal(scored["counts"], saved["counts"])
    for flags in (["--evaluate_3d_align_plane"], ["--evaluate_3d_align", "0.1", "--evaluate_3d_align_plane", "--evaluate_3d_align_scale"],
                  ["--evaluate_3d_align", "0.1", "--evaluate_3d_align_neighbours", "12"]):
        with pytest.raises(ValueError):
            run("refused", flags)

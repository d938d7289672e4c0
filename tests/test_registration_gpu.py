"""GPU: the registration (csrc/registration.hip, dvmvs.hip.registration) against the restatement of tests/registration_reference.py -- the
moments of an iteration, the transform, the solve and the whole loop bit for bit -- and the surface built on it: the aligned 3-D metrics,
``TSDFVolume.score_against`` and the program's ``--evaluate_3d_align``.  A restatement is computed once per case and never modified."""
import os

import numpy as np
import pytest
import torch

import nearest_reference as nr
import registration_reference as rr
import tsdf_fuse_scene as scene

pytestmark = pytest.mark.gpu

START = rr.rigid([0.3, -1.0, 0.5], 3.0, [0.02, 0.01, -0.03])                     # a T_0 that is not the identity: the transform takes part


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


def host(info):
    return {k: v.cpu().numpy() for k, v in info.items()}


def assert_record(got_T, got, want_T, want, label):
    """Everything the state block records against the restatement, bit for bit."""
    got = host(got)
    k = want["iterations"]
    assert int(got["iterations"]) == k and int(got["status"]) == want["status"], (label, got["iterations"], got["status"], want["status"])
    assert np.array_equal(got["inliers"][:k], want["inliers"]), label
    for key in ("fitness", "rmse"):
        assert bits(got[key][:k]) == bits(want[key]), (label, key, got[key][:k], want[key])
    assert bits(got["moments"]) == bits(want["moments"]), (label, got["moments"] - want["moments"])
    difference = np.abs(got_T.cpu().numpy() - want_T).max()
    assert bits(got_T.cpu().numpy()) == bits(want_T), f"{label}: T differs by {difference:.3e}"


# ---- one iteration ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4099, 66561])
def test_moments_of_one_iteration(hip_device, N):
    """One iteration from a T_0 that moves the points; max_distance trims none, about half and all of the pairs; the source starts 4 bytes
    off a 16-byte boundary; the call runs on a side stream.  N = 66561 gives 66 partial rows: lanes 0 and 1 of the solve add two each, and
    the last row holds one point."""
    from dvmvs.hip import registration
    rng = np.random.default_rng(3000 + N)
    target = rng.normal(size=(500, 3)).astype(np.float32)
    source = rng.normal(size=(N, 3)).astype(np.float32)
    dist = nr.nearest32(rr.transform32(source, START), target)[0]
    median = float(np.sort(dist)[N // 2])
    t_dev, s_dev = torch.from_numpy(target).to(hip_device), off_boundary(hip_device, source)
    for label, max_distance in (("none", float("inf")), ("half", median), ("all", float(dist.min()) * 0.5)):
        want_T, want = rr.icp(source, target, max_distance, init=START, max_iterations=1)
        expected = {"none": N, "half": int((dist <= np.float32(median)).sum()), "all": 0}[label]
        assert want["inliers"].tolist() == [expected]
        T, info = on_side_stream(hip_device, lambda: registration.icp(s_dev, t_dev, max_distance, init=START, max_iterations=1))
        assert T.dtype == torch.float64 and tuple(T.shape) == (4, 4) and T.is_cuda and all(v.is_cuda for v in info.values())
        assert_record(T, info, want_T, want, f"N={N} trim {label}")            # T too: the step composed onto START, or START itself


@pytest.mark.parametrize("N", [1, 257, 4099])
def test_transform_points(hip_device, N):
    from dvmvs.hip import registration
    points = np.random.default_rng(3100 + N).normal(size=(N, 3)).astype(np.float32) * np.float32(3.0)
    motion = rr.rigid([1.0, -2.0, 0.5], 37.0, [0.5, -1.5, 2.0], scale=1.3)
    want = rr.transform32(points, motion)
    T = torch.from_numpy(motion).to(hip_device)
    p = torch.from_numpy(points).to(hip_device)
    out = registration.transform_points(p, T)
    assert out.dtype == torch.float32 and out.data_ptr() != p.data_ptr() and bits(out.cpu().numpy()) == bits(want)
    assert bits(p.cpu().numpy()) == bits(points)
    given = torch.empty_like(p)
    assert registration.transform_points(p, T, out=given) is given and bits(given.cpu().numpy()) == bits(want)
    assert registration.transform_points(p, T, out=p) is p and bits(p.cpu().numpy()) == bits(want)                 # in place
    shifted = off_boundary(hip_device, points)
    assert bits(registration.transform_points(shifted, T).cpu().numpy()) == bits(want)


# ---- the solve -----------------------------------------------------------------------------------------------------------------------
def solve_cases():
    rng = np.random.default_rng(41)
    cloud = rng.normal(size=(400, 3)).astype(np.float32)
    moved = rr.transform32(cloud, rr.rigid([0.2, 1.0, -0.4], 4.0, [0.03, -0.02, 0.01])) + (rng.normal(size=(400, 3)) * 0.002).astype(np.float32)
    cases = [("random", moved, cloud, 0.5, False), ("random_scale", (moved / np.float32(1.05)).astype(np.float32), cloud, 0.5, True)]
    for name, source, target, max_distance, _ in rr.degenerate_cases():
        cases.append((name, source, target, max_distance, False))
    return cases


@pytest.mark.parametrize("case", solve_cases(), ids=lambda c: c[0])
def test_solve_on_the_device(hip_device, case):
    """T after ONE iteration: the float64 solve on the device against the restatement's, bit for bit."""
    from dvmvs.hip import registration
    name, source, target, max_distance, with_scale = case
    want_T, want = rr.icp(source, target, max_distance, max_iterations=1, with_scale=with_scale)
    T, info = registration.icp(torch.from_numpy(source).to(hip_device), torch.from_numpy(target).to(hip_device), max_distance, max_iterations=1,
                               with_scale=with_scale)
    print(f"{name}: status {int(info['status'])}, |T - restatement| {np.abs(T.cpu().numpy() - want_T).max():.3e}")
    assert_record(T, info, want_T, want, name)


# ---- the whole loop --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_scale", [False, True])
def test_whole_loop(hip_device, with_scale):
    from dvmvs import errors
    from dvmvs.hip import ops, registration
    source, target, (want_T, want) = rr.box_result(with_scale=with_scale)
    assert want["status"] == rr.CONVERGED
    s, t = torch.from_numpy(np.array(source)).to(hip_device), torch.from_numpy(np.array(target)).to(hip_device)
    T, info = registration.icp(s, t, 0.5, with_scale=with_scale)
    print(f"scale {with_scale}: {int(info['iterations'])} iterations, rmse {info['rmse'][:int(info['iterations'])].cpu().numpy()}")
    assert_record(T, info, want_T, want, f"box scale={with_scale}")
    longer, info60 = registration.icp(s, t, 0.5, with_scale=with_scale, max_iterations=60)       # the launches after convergence do nothing
    assert torch.equal(longer, T) and int(info60["iterations"]) == want["iterations"] and int(info60["status"]) == rr.CONVERGED
    again, _ = errors.register_points_device(s, t, 0.5, with_scale=with_scale, grid=ops.nearest_build(t))         # a grid the caller built
    assert torch.equal(again, T)
    if not with_scale:
        short_T, short = rr.icp(source, target, 0.5, max_iterations=3)
        got_T, got = registration.icp(s, t, 0.5, max_iterations=3)
        assert short["status"] == rr.LIMIT
        assert_record(got_T, got, short_T, short, "box, 3 iterations")


def test_nothing_is_read_by_the_call(hip_device):
    """With torch's synchronisation check set to raise, a registration, the transform and the selection of the last recorded iteration
    (as the program forms its one download) go through: they only enqueue."""
    from dvmvs.hip import registration
    source, target, _ = rr.box_case()
    s, t = torch.from_numpy(np.array(source)).to(hip_device), torch.from_numpy(np.array(target)).to(hip_device)
    registration.icp(s, t, 0.5)                                                   # the per-device workspaces exist from here on
    torch.cuda.synchronize(hip_device)
    torch.cuda.set_sync_debug_mode("error")
    try:
        T, info = registration.icp(s, t, 0.5)
        moved = registration.transform_points(s, T)
        last = (info["iterations"] - 1).clamp(min=0).reshape(1)
        packed = torch.cat([T.reshape(-1), info["status"].double().reshape(1), info["rmse"].index_select(0, last)])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert moved.shape == s.shape and packed.shape == (18,) and int(packed[16]) == rr.CONVERGED


def test_argument_checks(hip_device):
    from dvmvs.hip import registration
    cloud = torch.zeros((8, 3), device=hip_device)
    for bad in (dict(max_distance=0.0), dict(max_distance=float("nan")), dict(tolerance=-1.0), dict(tolerance=float("nan")),
                dict(max_iterations=0), dict(max_iterations=1025), dict(init=np.eye(3)), dict(init=np.full((4, 4), np.inf)),
                dict(init=torch.eye(4, device=hip_device)), dict(grid=torch.zeros(16, dtype=torch.uint8, device=hip_device))):
        with pytest.raises(ValueError):
            registration.icp(cloud, cloud, **{"max_distance": 0.1, **bad})
    for source, target in ((cloud[:0], cloud), (cloud, cloud[:0]), (cloud.double(), cloud), (cloud, cloud.reshape(-1))):
        with pytest.raises(ValueError):
            registration.icp(source, target, 0.1)
    with pytest.raises(ValueError):
        registration.transform_points(cloud, torch.eye(4, device=hip_device))                  # float32 T
    state = registration.icp_workspace(hip_device, 1000, 30)
    assert state.dtype == torch.float64 and state.is_cuda and state.numel() * 8 == 1024 + 12032 + 2 * 4096 + 256


# ---- the aligned metrics ---------------------------------------------------------------------------------------------------------------
OFFSET = rr.rigid([0.4, 1.0, -0.3], 1.0, np.array([0.012, -0.01, 0.0125]))      # 1 degree and 2 cm (|t| = 0.02)


def fused(dev, frame_ids):
    from dvmvs.tsdf import TSDFVolume
    depth, rgb = scene.frames()
    poses = scene.poses()
    vol = TSDFVolume(scene.BOUNDS.copy(), scene.VOXEL, device=dev)
    vol.integrate_frames(rgb[frame_ids], depth[frame_ids], scene.K, poses[frame_ids])
    return vol


def test_score_against_with_alignment(hip_device):
    """A small fused volume against its own vertices moved by the inverse of OFFSET: the fused surface is the reference moved by 1 degree
    and 2 cm.  Unaligned, precision at 1 cm is below a half; aligned, every point is within it."""
    from dvmvs import errors
    assert abs(np.linalg.norm(OFFSET[:3, 3]) - 0.02) < 1e-3
    vol = fused(hip_device, [0, 1])
    verts = vol.vertices().cpu().numpy()
    reference = (verts.astype(np.float64) @ np.linalg.inv(OFFSET)[:3, :3].T + np.linalg.inv(OFFSET)[:3, 3]).astype(np.float32)
    plain = vol.score_against(reference, threshold=0.01).cpu().numpy()
    row, sizes, T = vol.score_against(reference, threshold=0.01, return_sizes=True, align_distance=0.1, return_transform=True)
    assert T.is_cuda and T.dtype == torch.float64 and tuple(T.shape) == (4, 4) and sizes == (len(verts), len(verts))
    row, T = row.cpu().numpy(), T.cpu().numpy()
    print(f"{len(verts)} vertices: unaligned {plain}, aligned {row}, |T - inverse motion| {np.abs(T - np.linalg.inv(OFFSET)).max():.2e}")
    assert plain[3] < 0.5
    assert row[3] == 1.0 and row[0] < 1e-4
    assert np.abs(T - np.linalg.inv(OFFSET)).max() < 1e-4
    want, want_T = errors.compute_reconstruction_errors(verts, reference, 0.01, align_distance=0.1, return_transform=True)
    assert bits(row) == bits(want), (row, want)
    assert bits(T) == bits(want_T)
    # the module-level device function, and a scale that it finds to be 1
    dev_row = errors.compute_reconstruction_errors_device(torch.from_numpy(verts).to(hip_device), torch.from_numpy(reference).to(hip_device), 0.01,
                                                          align_distance=0.1)
    assert bits(dev_row.cpu().numpy()) == bits(row)
    _, scaled_T = vol.score_against(reference, threshold=0.01, align_distance=0.1, align_scale=True, return_transform=True)
    assert abs(np.cbrt(np.linalg.det(scaled_T.cpu().numpy()[:3, :3])) - 1.0) < 1e-4
    # without the keywords nothing changes
    assert bits(vol.score_against(reference, threshold=0.01, align_distance=None).cpu().numpy()) == bits(plain)


# ---- the program -------------------------------------------------------------------------------------------------------------------------
def test_program_aligns(hip_device, golden_dir, tmp_path):
    """``python -m dvmvs.tsdf --evaluate_3d --evaluate_3d_align 0.1`` on the two keyframes of the sample scene: the extra keys; without the
    flag two runs write the same bytes with the keys they always had; ``--groundtruth_transform`` brings a displaced mesh back."""
    from PIL import Image
    from dvmvs.dataset_loader import load_depth_png, resize_nearest
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

    def run(tag, flags):
        out = tmp_path / tag
        main(["--reconstruction_folder", str(out), "--prediction_folder", str(tmp_path / "pred"), "--data_folder", str(tmp_path / "data"),
              "--voxel_size", "0.05", "--evaluate_3d", "--threshold_3d", "0.1"] + flags)
        return {w: open(out / w, "rb").read() for w in sorted(os.listdir(out))}

    plain, again, aligned = run("plain", []), run("again", []), run("aligned", ["--evaluate_3d_align", "0.1"])
    assert plain == again and len(plain) == 2
    mesh_file, = [w for w in plain if w.endswith("_complete.ply")]
    errors_file, = [w for w in plain if w.endswith("_errors3d.npz")]
    saved = np.load(tmp_path / "plain" / errors_file)
    assert sorted(saved.files) == ["arr_0", "counts", "names", "threshold"]
    assert set(aligned) == set(plain) and aligned[mesh_file] == plain[mesh_file]
    scored = np.load(tmp_path / "aligned" / errors_file)
    assert sorted(scored.files) == sorted(saved.files + ["transform", "align_iterations", "align_status", "align_fitness", "align_rmse"])
    T = scored["transform"]
    print(f"aligned run: row {scored['arr_0']} (plain {saved['arr_0']}), {scored['align_iterations']} iterations, status {scored['align_status']}, "
          f"fitness {scored['align_fitness']}, rmse {scored['align_rmse']}")
    assert T.dtype == np.float64 and T.shape == (4, 4) and np.isfinite(T).all() and T[3].tolist() == [0, 0, 0, 1]
    assert abs(np.linalg.det(T[:3, :3]) - 1.0) < 1e-9
    assert 1 <= scored["align_iterations"] <= 30 and scored["align_status"] in (1, 3)
    assert 0.0 < scored["align_fitness"] <= 1.0 and 0.0 <= scored["align_rmse"] <= 0.1
    assert scored["arr_0"].dtype == np.float32 and np.array_equal(scored["counts"], saved["counts"])
    # a ground-truth mesh in a frame of its own: the system's mesh displaced by the inverse of OFFSET, and the file that brings it back
    verts, faces = TSDFFusion.meshread(str(tmp_path / "plain" / mesh_file))
    away = np.linalg.inv(OFFSET)
    displaced = (verts.astype(np.float64) @ away[:3, :3].T + away[:3, 3]).astype(np.float32)
    TSDFFusion.meshwrite(str(tmp_path / "gt.ply"), displaced, faces, np.zeros_like(displaced), np.zeros(displaced.shape, np.uint8))
    np.savetxt(tmp_path / "offset.txt", OFFSET)
    back = run("back", ["--groundtruth_mesh", str(tmp_path / "gt.ply"), "--groundtruth_transform", str(tmp_path / "offset.txt")])
    assert back[mesh_file] == plain[mesh_file]
    row = np.load(tmp_path / "back" / errors_file)["arr_0"]
    print(f"ground truth brought back by its transform file: {row}")
    assert row[0] < 1e-5 and row[1] < 1e-5 and row[3] == 1.0 and row[4] == 1.0

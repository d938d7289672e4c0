"""GPU: the nearest-point op (csrc/nearest_points.hip) against the float32 brute force of tests/nearest_reference.py -- distances
bit-identical, indices the smallest minimiser, in every case -- and the 3-D reconstruction metrics built on it, up to the program's
``--evaluate_3d``.  A brute-force reference is computed once per case and never modified."""
import functools
import os

import numpy as np
import pytest
import torch

import nearest_reference as nr
import tsdf_fuse_scene as scene

pytestmark = pytest.mark.gpu


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def gaussian(n, seed):
    return f32(np.random.default_rng(seed).normal(size=(n, 3)))


def device_nearest(dev, query, target):
    from dvmvs.hip import ops
    dist, index = ops.nearest_distance(torch.tensor(query, device=dev), torch.tensor(target, device=dev), return_index=True)
    assert dist.dtype == torch.float32 and index.dtype == torch.int32 and dist.shape == index.shape == (len(query),)
    return dist.cpu().numpy(), index.cpu().numpy()


def assert_exact(dev, query, target, label):
    """dist bit-identical to the float32 brute force, index the smallest minimiser."""
    query, target = f32(query), f32(target)
    want_d, want_i = nr.nearest32(query, target)
    got_d, got_i = device_nearest(dev, query, target)
    bad = np.flatnonzero(got_d.view(np.int32) != want_d.view(np.int32))
    assert bad.size == 0, f"{label}: {bad.size} of {len(query)} distances differ, first at {bad[0]}: {got_d[bad[0]]!r} != {want_d[bad[0]]!r}"
    bad = np.flatnonzero(got_i != want_i)
    assert bad.size == 0, f"{label}: {bad.size} indices differ, first at {bad[0]}: {got_i[bad[0]]} != {want_i[bad[0]]}"
    return got_d, got_i


@pytest.mark.parametrize("M", [1, 2, 65, 1000])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 1000])
def test_gaussian_clouds(hip_device, N, M):
    assert_exact(hip_device, gaussian(N, 1000 + N), gaussian(M, 2000 + M), f"N={N} M={M}")


def on_and_off(target, seed):
    """Queries on the set (some of its points) and off it."""
    rng = np.random.default_rng(seed)
    return np.concatenate([target[rng.integers(0, len(target), 40)], gaussian(90, seed + 1)])


def test_coincident_targets(hip_device):
    target = np.repeat(f32([[0.3, -1.2, 2.5]]), 77, axis=0)
    dist, index = assert_exact(hip_device, on_and_off(target, 11), target, "coincident")
    assert (index == 0).all() and (dist[:40] == 0).all()


def test_coplanar_targets(hip_device):
    target = gaussian(500, 12)
    target[:, 2] = 0.75
    assert_exact(hip_device, on_and_off(target, 13), target, "coplanar")


def test_collinear_targets(hip_device):
    target = np.zeros((300, 3), np.float32)
    target[:, 0] = np.random.default_rng(14).normal(size=300)
    target[:, 1], target[:, 2] = -0.5, 2.0
    assert_exact(hip_device, on_and_off(target, 15), target, "collinear")


def test_regular_lattice(hip_device):
    """Targets on a regular lattice that spans the box; queries at lattice points, between them and one float32 step off them.  (Where
    this lattice lies relative to the grid's cells is up to the header; ``test_targets_on_cell_faces`` places points ON the faces.)"""
    g = np.arange(9, dtype=np.float32) * np.float32(0.125)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    some = lattice[::7]
    up = np.nextafter(some, np.float32(10.0)).astype(np.float32)
    down = np.nextafter(some, np.float32(-10.0)).astype(np.float32)
    mixed = some.copy()
    mixed[:, 0], mixed[:, 2] = up[:, 0], down[:, 2]
    centres = lattice[::5] + np.float32(0.0625)
    assert_exact(hip_device, np.concatenate([lattice, centres, up, down, mixed]), lattice, "lattice")


def test_targets_on_cell_faces(hip_device):
    """Targets ON the faces of the grid the device built: a provisional cloud with the case's box and size is built, its header read
    back, and the targets are placed at the smallest float32 coordinate of each drawn cell on all three axes (one step below lies the
    cell before: asserted with the device's header).  Queries: those points, one float32 step either side on every axis, mixed, and
    cell centres."""
    import nearest_grid_emulation as emu
    from dvmvs.hip import ops
    header = ops.nearest_grid_header(ops.nearest_build(torch.tensor(emu.provisional_cloud(), device=hip_device)))
    assert header["inv_h"] > 0 and (header["dim"] >= 3).all() and header["ncells"] == int(np.prod(header["dim"]))
    query, target, ks = emu.face_case(header)
    emu.assert_on_faces(header, target[8:], ks)
    integral = sum(int((emu.scaled(header, target[8:, a], a) == ks[:, a]).sum()) for a in range(3))
    print(f"device grid {header['dim']}, inv_h {header['inv_h']!r}: {len(target) - 8} targets on faces, {integral} coordinates with an integral s")
    assert integral > 0
    again = ops.nearest_grid_header(ops.nearest_build(torch.tensor(target, device=hip_device)))      # the same box and M: the same grid
    assert all(np.array_equal(header[key], again[key]) for key in header)
    assert_exact(hip_device, query, target, "faces")


def test_differences_that_underflow(hip_device):
    """Two distinct targets 1e-23 apart at the corner of a box of 1e-12: their squared distance underflows to 0, so each is at distance
    0 from both and the index is the smaller one."""
    rng = np.random.default_rng(27)
    target = f32(np.concatenate([rng.uniform(0, 1e-12, size=(100, 3)), [[0.0, 0.0, 0.0], [1e-23, 0.0, 0.0]]]))
    assert not np.array_equal(target[-1], target[-2])
    dist, index = assert_exact(hip_device, np.concatenate([target[-2:], target[:20]]), target, "underflow")
    assert dist[:2].tolist() == [0, 0] and index[:2].tolist() == [100, 100]


def test_two_distant_clusters(hip_device):
    """Two tight clusters 50 units apart: queries between them cross many empty cells, so a premature stop of the ring search shows."""
    rng = np.random.default_rng(16)
    a = f32(rng.normal(size=(150, 3)) * 0.01)
    b = f32(rng.normal(size=(150, 3)) * 0.01 + np.array([50.0, 0.0, 0.0]))
    line = np.zeros((101, 3), np.float32)
    line[:, 0] = np.linspace(0.0, 50.0, 101)                     # holds the midpoint x = 25
    off_line = line + f32(rng.normal(size=(101, 3)) * 0.5)
    oblique = f32(rng.normal(size=(150, 3)) * 0.01 + np.array([30.0, 40.0, 0.0]))       # a second pair, not along an axis
    assert_exact(hip_device, np.concatenate([line, off_line]), np.concatenate([a, b]), "clusters along x")
    assert_exact(hip_device, np.concatenate([line, off_line, line[:, [1, 0, 2]]]), np.concatenate([a, oblique]), "oblique clusters")


def test_queries_far_outside_the_box(hip_device):
    target = f32(np.random.default_rng(17).uniform(-1.0, 1.0, size=(800, 3)))
    extent = 2.0
    queries = []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            q = np.random.default_rng(18 + axis).uniform(-1.0, 1.0, size=(5, 3))
            q[:, axis] = sign * 10.0 * extent
            queries.append(q)
    queries.append(np.array([[20.0, 20.0, 20.0], [-20.0, 20.0, -20.0], [20.0, -20.0, 0.3]]))
    assert_exact(hip_device, np.concatenate(queries), target, "outside")


def test_duplicate_targets(hip_device):
    rng = np.random.default_rng(19)
    base = gaussian(200, 20)
    target = np.repeat(base, 3, axis=0)[rng.permutation(600)]
    dist, index = assert_exact(hip_device, np.concatenate([base, gaussian(100, 21)]), target, "duplicates")
    first = {}
    for j, t in enumerate(target):
        first.setdefault(t.tobytes(), j)
    assert (dist[:200] == 0).all() and [first[b.tobytes()] for b in base] == index[:200].tolist()


@functools.lru_cache(maxsize=None)
def large_case():
    """M = 100 003 targets near a 2-D sheet (as a mesh's vertices are), N = 4 096 queries: half near the sheet, half uniform in the box.
    The grid has more cells than one workgroup of the scan takes.  The brute force is 4e8 pairs, chunked; computed once."""
    rng = np.random.default_rng(22)

    def sheet(n, noise):
        xy = rng.uniform(-1.0, 1.0, size=(n, 2))
        z = 0.3 * np.sin(3.0 * xy[:, 0]) * np.cos(2.0 * xy[:, 1]) + rng.normal(size=n) * noise
        return f32(np.column_stack([xy, z]))

    target = sheet(100003, 0.002)
    query = np.concatenate([sheet(2048, 0.01), f32(rng.uniform(-1.0, 1.0, size=(2048, 3)) * np.array([1.0, 1.0, 0.4]))])
    want = nr.nearest32(query, target)
    for a in (target, query) + want:
        a.setflags(write=False)
    return query, target, want


def test_large_sheet(hip_device):
    query, target, (want_d, want_i) = large_case()
    got_d, got_i = device_nearest(hip_device, query, target)
    assert np.array_equal(got_d.view(np.int32), want_d.view(np.int32)) and np.array_equal(got_i, want_i)


def test_repeatable_on_any_stream_and_in_place(hip_device):
    from dvmvs.hip import ops
    query, target, (want_d, want_i) = large_case()
    q, t = torch.tensor(query, device=hip_device), torch.tensor(target, device=hip_device)      # (copies: the cached arrays are read-only)
    first = ops.nearest_distance(q, t, return_index=True)
    second = ops.nearest_distance(q, t, return_index=True)
    assert np.array_equal(first[0].cpu().numpy().view(np.int32), want_d.view(np.int32)) and np.array_equal(first[1].cpu().numpy(), want_i)
    assert torch.equal(first[0].view(torch.int32), second[0].view(torch.int32)) and torch.equal(first[1], second[1])
    side = torch.cuda.Stream(device=hip_device)
    side.wait_stream(torch.cuda.current_stream(hip_device))
    with torch.cuda.stream(side):
        third = ops.nearest_distance(q, t, return_index=True)
    side.synchronize()
    torch.cuda.current_stream(hip_device).wait_stream(side)
    assert torch.equal(first[0].view(torch.int32), third[0].view(torch.int32)) and torch.equal(first[1], third[1])
    assert ops.nearest_distance(q, t).dtype == torch.float32                      # without the index
    # query and target may be the same tensor: every distance 0, the index of the first duplicate (here: the point itself)
    same = torch.from_numpy(np.concatenate([gaussian(300, 23)] * 2)).to(hip_device)
    dist, index = ops.nearest_distance(same, same, return_index=True)
    assert bool((dist == 0).all()) and index.cpu().tolist() == list(range(300)) * 2


def test_op_argument_checks(hip_device):
    from dvmvs.hip import ops
    q = torch.zeros((4, 3), device=hip_device)
    empty = torch.zeros((0, 3), device=hip_device)
    dist, index = ops.nearest_distance(empty, q, return_index=True)               # N = 0: nothing to do
    assert dist.shape == (0,) and index.shape == (0,)
    for bad_q, bad_t in ((q, empty), (q.double(), q), (q, q.double()), (q.reshape(3, 4), q), (q, q.reshape(-1))):
        with pytest.raises(ValueError):
            ops.nearest_distance(bad_q, bad_t)
    with pytest.raises(RuntimeError):
        ops.nearest_distance(q.cpu(), q)
    d = torch.zeros(5, device=hip_device)
    for a, b, kwargs in ((d[:0], d, {}), (d, d.double(), {}), (d.reshape(5, 1), d, {}), (d, d, dict(threshold=float("nan"))),
                         (d, d, dict(out=torch.zeros(5, device=hip_device))), (d, d, dict(counts=torch.zeros(2, device=hip_device)))):
        with pytest.raises(ValueError):
            ops.distance_metrics(a, b, **kwargs)
    with pytest.raises(RuntimeError):
        ops.distance_metrics(d.cpu(), d)


# ---- metrics ------------------------------------------------------------------------------------------------------------------------------
def check_row(row, counts, pred, gt, threshold, exact=False):
    """The device row against dvmvs.errors.compute_reconstruction_errors on the same (host) clouds."""
    from dvmvs import errors
    want = errors.compute_reconstruction_errors(pred, gt, threshold)
    dist_pred, dist_gt = errors.nearest_distances(pred, gt), errors.nearest_distances(gt, pred)
    want_counts = errors.reconstruction_metrics_from_distances(dist_pred, dist_gt, threshold)[1]
    print(f"device {row}  host {want}  counts {counts} of {len(pred)}, {len(gt)}")
    assert row.dtype == np.float32 and row.shape == (6,) and np.isfinite(row).all()
    assert np.array_equal(counts, want_counts)                                    # bit-identical distances: equal integers
    assert row[3] == np.float32(counts[0] / len(pred)) and row[4] == np.float32(counts[1] / len(gt))
    assert (nr.ulps(row[:2], want[:2]) <= 1).all()                                # the fp64 sum and fsum can differ in the last rounding
    assert nr.ulps(row[2], np.float32((np.float64(row[0]) + np.float64(row[1])) / 2.0)) <= 1
    p, r = np.float64(row[3]), np.float64(row[4])
    assert nr.ulps(row[5], np.float32(2.0 * p * r / (p + r) if p + r > 0 else 0.0)) <= 1
    if exact:
        assert np.array_equal(row, want)


def device_row(dev, pred, gt, threshold):
    from dvmvs import errors
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    row = errors.compute_reconstruction_errors_device(torch.from_numpy(f32(pred)).to(dev), torch.from_numpy(f32(gt)).to(dev), threshold, counts=counts)
    assert row.is_cuda and row.dtype == torch.float32 and tuple(row.shape) == (6,)
    return row.cpu().numpy(), counts.cpu().numpy()


@pytest.mark.parametrize("threshold", [0.05, 0.25])
def test_metrics_against_the_host_function(hip_device, threshold):
    rng = np.random.default_rng(24)
    pred = gaussian(3000, 25)
    gt = np.concatenate([pred[:1200] + f32(rng.normal(size=(1200, 3)) * 0.03), gaussian(1500, 26)])
    row, counts = device_row(hip_device, pred, gt, threshold)
    check_row(row, counts, pred, gt, threshold)


@pytest.mark.parametrize("case", nr.hand_cases(), ids=lambda c: c[0])
def test_metrics_of_hand_computed_clouds(hip_device, case):
    _, pred, gt, threshold, expected = case
    row, counts = device_row(hip_device, pred, gt, threshold)
    assert np.array_equal(row, np.array(expected, dtype=np.float32)), row         # (their sums are exact in float64: no last-bit slack)
    check_row(row, counts, pred, gt, threshold, exact=True)


def test_empty_clouds_raise_on_the_device_path(hip_device):
    from dvmvs import errors
    some, none = torch.zeros((3, 3), device=hip_device), torch.zeros((0, 3), device=hip_device)
    for pred, gt in ((none, some), (some, none)):
        with pytest.raises(ValueError):
            errors.compute_reconstruction_errors_device(pred, gt)


# ---- TSDFVolume.score_against -------------------------------------------------------------------------------------------------------------
def fused(dev, frame_ids):
    from dvmvs.tsdf import TSDFVolume
    depth, rgb = scene.frames()
    poses = scene.poses()
    vol = TSDFVolume(scene.BOUNDS.copy(), scene.VOXEL, device=dev)
    vol.integrate_frames(rgb[frame_ids], depth[frame_ids], scene.K, poses[frame_ids])
    return vol


def test_score_against(hip_device):
    from dvmvs import errors
    full, half = fused(hip_device, [0, 1, 2, 3, 4, 5]), fused(hip_device, [0, 2, 4])
    itself = full.score_against(full)
    assert itself.is_cuda and itself.cpu().tolist() == [0, 0, 0, 1, 1, 1]
    pred, gt = full.get_mesh()[0], half.get_mesh()[0]
    assert len(pred) > 100 and len(gt) > 100 and len(pred) != len(gt)
    want = errors.compute_reconstruction_errors(pred, gt, 0.05)
    row = full.score_against(half).cpu().numpy()
    print(f"{len(pred)} vertices against {len(gt)}: device {row}, host {want}")
    assert (nr.ulps(row[:3], want[:3]) <= 1).all() and np.array_equal(row[3:5], want[3:5]) and nr.ulps(row[5], want[5]) <= 1
    for reference in (torch.from_numpy(gt).to(hip_device), torch.from_numpy(gt), gt, gt.astype(np.float64)):
        assert np.array_equal(full.score_against(reference).cpu().numpy(), row)
    tight = errors.compute_reconstruction_errors(pred, gt, 0.02)                  # the threshold reaches the kernel
    assert np.array_equal(full.score_against(half, threshold=0.02).cpu().numpy()[3:5], tight[3:5])
    from dvmvs.tsdf import TSDFVolume
    with pytest.raises(ValueError):
        full.score_against(TSDFVolume(scene.BOUNDS.copy(), scene.VOXEL, device=hip_device))      # nothing fused: no vertex
    with pytest.raises(ValueError):
        full.score_against(np.zeros((5, 2), np.float32))


def test_score_against_of_a_live_fusion(hip_device):
    from dvmvs.tsdf import LiveFusion
    depth, rgb = scene.frames()
    poses = scene.poses()
    live = LiveFusion(scene.BOUNDS.copy(), voxel_size=scene.VOXEL, max_depth=5.0, batch=4, device=hip_device)
    for i in range(6):
        live.add(torch.from_numpy(depth[i]).to(hip_device), rgb[i], scene.K, poses[i])
    full = fused(hip_device, [0, 1, 2, 3, 4, 5])
    assert live.volume.score_against(full).cpu().tolist() == [0, 0, 0, 1, 1, 1]
    half = fused(hip_device, [0, 2, 4])
    assert torch.equal(live.volume.score_against(half), full.score_against(half))


# ---- the program ----------------------------------------------------------------------------------------------------------------------------
def test_program_evaluates_in_3d(hip_device, golden_dir, tmp_path):
    """``python -m dvmvs.tsdf --evaluate_3d`` on two keyframes of the sample scene (their depth maps as 'predictions', 5 cm voxels): the
    output folder holds what the plain run wrote, byte for byte, and the one ``_errors3d.npz``."""
    from PIL import Image
    from dvmvs.dataset_loader import load_depth_png, resize_nearest
    from dvmvs.errors import RECONSTRUCTION_METRICS
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
    written = {}
    for tag, flag in (("plain", []), ("scored", ["--evaluate_3d", "--threshold_3d", "0.1"]),
                      ("both", ["--evaluate_3d", "--threshold_3d", "0.1", "--save_groundtruth"])):
        out = tmp_path / tag
        main(["--reconstruction_folder", str(out), "--prediction_folder", str(tmp_path / "pred"), "--data_folder", str(tmp_path / "data"),
              "--voxel_size", "0.05"] + flag)
        written[tag] = {w: open(out / w, "rb").read() for w in sorted(os.listdir(out))}
    assert len(written["plain"]) == 1
    (mesh_file, mesh_bytes), = written["plain"].items()
    assert mesh_file.endswith("_complete.ply")
    errors_file = mesh_file[:-len("_complete.ply")] + "_errors3d.npz"
    assert set(written["scored"]) == {mesh_file, errors_file} and written["scored"][mesh_file] == mesh_bytes
    saved = np.load(tmp_path / "scored" / errors_file)
    row, counts = saved["arr_0"], saved["counts"]
    print(f"3-D metrics of the two-keyframe reconstruction at 0.1 m: {dict(zip(RECONSTRUCTION_METRICS, row.tolist()))}, vertices {counts}")
    assert tuple(saved["names"].tolist()) == RECONSTRUCTION_METRICS and saved["threshold"] == np.float32(0.1)
    assert row.dtype == np.float32 and row.shape == (6,) and np.isfinite(row).all() and (row[:3] >= 0).all()
    assert ((row[3:] >= 0) & (row[3:] <= 1)).all()
    assert nr.ulps(row[2], np.float32((np.float64(row[0]) + np.float64(row[1])) / 2.0)) <= 1
    assert counts.dtype == np.int64 and counts.shape == (2,) and counts[1] > 0
    assert f"element vertex {counts[0]}\n" in mesh_bytes[:400].decode()
    # with --save_groundtruth as well: the same meshes and row, and the ground-truth mesh has counts[1] vertices
    groundtruth_file, = [w for w in written["both"] if "GROUNDTRUTH" in w]
    assert set(written["both"]) == {mesh_file, errors_file, groundtruth_file} and written["both"][mesh_file] == mesh_bytes
    assert f"element vertex {counts[1]}\n" in written["both"][groundtruth_file][:400].decode()
    both = np.load(tmp_path / "both" / errors_file)
    assert np.array_equal(both["arr_0"], row) and np.array_equal(both["counts"], counts)
    # what the host function says on vertices obtained through the public API: the two fusions of the program, repeated here
    from dvmvs.dataset_loader import PreprocessImage, load_image
    from dvmvs.errors import compute_reconstruction_errors
    from dvmvs.tsdf import TSDFFusion, TSDFVolume
    K = np.loadtxt(scene_dir / "K.txt").astype(np.float32)
    poses = np.fromfile(str(scene_dir / "poses.txt"), dtype=float, sep="\n ").reshape((-1, 4, 4))
    images = [load_image(str(scene_dir / "images" / n)) for n in names]
    pre = PreprocessImage(K=K, old_width=images[0].shape[1], old_height=images[0].shape[0], new_width=320, new_height=256, distortion_crop=0,
                          perform_crop=False)
    scaled_K = pre.get_updated_intrinsics()
    masked = preds.copy()
    masked[masked > 5.0] = 0.0
    bounds = TSDFFusion.calculate_volume_bounds(list(masked), list(poses), scaled_K) * 1.05
    predicted, groundtruth = (TSDFVolume(bounds.copy(), voxel_size=0.05, device=hip_device) for _ in range(2))
    for image, prediction, name, pose in zip(images, masked, names, poses):
        predicted.integrate(resize_nearest(image, 320, 256).astype(np.uint8), prediction, scaled_K, pose)
        depth = load_depth_png(str(scene_dir / "depth" / name))
        depth[depth > 5.0] = 0.0
        groundtruth.integrate(image.astype(np.uint8), depth, K, pose)
    pred_vertices, gt_vertices = predicted.get_mesh()[0], groundtruth.get_mesh()[0]
    assert [len(pred_vertices), len(gt_vertices)] == counts.tolist()
    want = compute_reconstruction_errors(pred_vertices, gt_vertices, 0.1)
    print(f"host function on the same vertices: {want}")
    assert (nr.ulps(row[:3], want[:3]) <= 1).all() and np.array_equal(row[3:5], want[3:5]) and nr.ulps(row[5], want[5]) <= 1
    assert not np.array_equal(row, compute_reconstruction_errors(gt_vertices, pred_vertices, 0.1))       # the roles are not swapped

"""Batched TSDF fusion on the GPU (csrc/tsdf_fuse.hip, TSDFVolume.integrate_frames, dvmvs.tsdf.LiveFusion, the runners' ``fuse=``).  Nothing
here has a tolerance: every comparison is ``torch.equal`` against the per-frame kernel (``TSDFVolume.integrate``), which tests/test_tsdf.py
holds to the CPU oracle and the reference's fixture."""
import os

import numpy as np
import pytest
import torch

import synthetic as syn
import tsdf_fuse_scene as scene

pytestmark = pytest.mark.gpu


def fresh(dev):
    from dvmvs.tsdf import TSDFVolume
    return TSDFVolume(scene.BOUNDS.copy(), scene.VOXEL, device=dev)


def volumes(vol):
    return vol._tsdf, vol._weight, vol._color


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(volumes(a), volumes(b)))


def sequential(dev, depth, rgb, K, poses, weights=None):
    """The yardstick: one ``integrate`` call per frame, in order."""
    vol = fresh(dev)
    for i in range(len(depth)):
        vol.integrate(rgb[i], depth[i], K, poses[i], obs_weight=1.0 if weights is None else weights[i])
    return vol


@pytest.fixture(scope="module")
def six(hip_device):
    """The six frames, and the volume six ``integrate`` calls make of them (shared, never modified)."""
    depth, rgb = scene.frames()
    poses = scene.poses()
    return depth, rgb, poses, sequential(hip_device, depth, rgb, scene.K, poses)


@pytest.mark.parametrize("splits", [(6,), (1, 5), (3, 3)])
def test_batch_equals_sequence(hip_device, six, splits):
    depth, rgb, poses, want = six
    got, first = fresh(hip_device), 0
    for n in splits:
        got.integrate_frames(rgb[first:first + n], depth[first:first + n], scene.K, poses[first:first + n])
        first += n
    assert int((want._weight > 0).sum()) >= 7000        # not two untouched volumes
    assert same(got, want)


def test_batch_equals_sequence_with_a_weight_per_frame(hip_device, six):
    depth, rgb, poses, _ = six
    weights = [1.0, 2.0, 0.5, 3.0, 1.5, 0.25]
    want = sequential(hip_device, depth, rgb, scene.K, poses, weights)
    got = fresh(hip_device)
    got.integrate_frames(rgb, depth, scene.K, poses, obs_weight=weights)
    assert int((want._weight > 0).sum()) >= 7000 and same(got, want)


def test_batch_equals_sequence_for_one_view_five_times(hip_device, six):
    """Five different depth maps from the same pose: every observed voxel carries a running mean of up to five terms."""
    depth, rgb, poses, _ = six
    front = np.repeat(poses[:1], 5, axis=0)
    want = sequential(hip_device, depth[:5], rgb[:5], scene.K, front)
    got = fresh(hip_device)
    got.integrate_frames(rgb[:5], depth[:5], np.repeat(scene.K[None], 5, axis=0), front)
    assert int((want._weight > 0).sum()) >= 7000 and float(want._weight.max()) == 5.0 and same(got, want)


def test_more_frames_than_one_launch_takes(hip_device):
    """70 frames of 16x20: the launcher splits them into 64 + 6, in order."""
    n, h, w = 70, 16, 20
    depth, rgb = scene.frames(n, h, w, seed=1)
    base = scene.poses()
    poses = np.stack([base[i % 6] for i in range(n)])
    poses[:, :3, 3] += 0.01 * (np.arange(n) // 6)[:, None] * np.array([1.0, -0.5, 0.25], dtype=np.float32)
    K = scene.scaled_K(h, w)
    want = sequential(hip_device, depth, rgb, K, poses)
    got = fresh(hip_device)
    got.integrate_frames(rgb, depth, K, poses)
    assert int((want._weight > 0).sum()) >= 7000 and same(got, want)


def test_non_finite_depths(hip_device, six):
    """A NaN depth is integrated with dist = 1 by the dense kernel (every comparison with NaN is false) and +inf with dist = 1 too: the
    frame must get no far plane."""
    depth, rgb, poses, _ = six
    d = depth[:1].copy()
    d[0, 5, 5], d[0, 6, 7] = np.nan, np.inf
    want = sequential(hip_device, d, rgb[:1], scene.K, poses[:1])
    got = fresh(hip_device)
    got.integrate_frames(rgb[:1], d, scene.K, poses[:1])
    assert same(got, want)
    # the NaN pixel's voxels were integrated, out to the far end of its ray: more voxels than the finite frame observes
    finite = sequential(hip_device, depth[:1], rgb[:1], scene.K, poses[:1])
    assert int((want._weight > 0).sum()) > int((finite._weight > 0).sum())


def test_all_zero_depth(hip_device, six):
    _, rgb, poses, _ = six
    got = fresh(hip_device)
    stats = got.integrate_frames(rgb[:1], np.zeros((1, scene.HEIGHT, scene.WIDTH), np.float32), scene.K, poses[:1], stats=True)
    assert same(got, fresh(hip_device)) and same(got, sequential(hip_device, np.zeros((1, scene.HEIGHT, scene.WIDTH), np.float32), rgb[:1],
                                                                 scene.K, poses[:1]))
    assert stats.tolist() == [0, 0]        # nothing to integrate anywhere: no tile loads the volume


def test_max_depth_equals_the_host_mask(hip_device, six):
    depth, rgb, poses, _ = six
    masked = depth.copy()
    masked[masked > 1.4] = 0.0
    assert 0 < int((masked != depth).sum()) < depth.size
    want = sequential(hip_device, masked, rgb, scene.K, poses)
    got = fresh(hip_device)
    got.integrate_frames(rgb, depth, scene.K, poses, max_depth=1.4)
    assert same(got, want) and not same(got, six[3])


def test_folded_colour_equals_8_bit_colour(hip_device, six):
    from dvmvs.tsdf import fold_color
    depth, rgb, poses, want = six
    folded = torch.from_numpy(np.stack([fold_color(c) for c in rgb])).to(hip_device)
    got = fresh(hip_device)
    got.integrate_frames(folded, depth, scene.K, poses)
    assert same(got, want)


def test_culling_happens_and_is_counted(hip_device, six):
    from dvmvs.hip import ops
    depth, rgb, poses, _ = six
    tiles = ops.tsdf_fuse_tile_count(scene.DIMS)
    index = {name: i for i, name in enumerate(scene.POSE_NAMES)}

    def run(names):
        ids = [index[n] for n in names]
        vol = fresh(hip_device)
        stats = vol.integrate_frames(rgb[ids], depth[ids], scene.K, poses[ids], stats=True)
        return vol, stats.tolist()

    vol, stats = run(["away", "far"])
    assert stats == [0, 0] and same(vol, fresh(hip_device))
    _, (kept, loaded) = run(["graze"])
    assert 0 < kept < tiles and loaded == kept
    _, (kept, loaded) = run(scene.POSE_NAMES)
    assert 0 < kept < 6 * tiles and 0 < loaded <= tiles
    # the tile count of the Python side is the kernel's: a view that sees every voxel, with a NaN depth (no far plane), keeps every tile
    all_seeing = scene.translation(0.0, 0.0, -60.0).astype(np.float32)[None]
    nan = np.full((1, scene.HEIGHT, scene.WIDTH), np.nan, np.float32)
    stats = fresh(hip_device).integrate_frames(rgb[:1], nan, scene.K, all_seeing, stats=True)
    assert stats.tolist() == [tiles, tiles]


def test_live_fusion_with_a_pending_frame(hip_device):
    """9 frames through ``add`` with batch = 4: two launches and one frame pending, which ``volume`` flushes.  The loop runs with PyTorch's
    synchronisation detector armed."""
    from dvmvs.tsdf import LiveFusion
    n = 9
    depth, rgb = scene.frames(n, seed=2)
    base = scene.poses()
    poses = np.stack([base[(0, 1, 4)[i % 3]] for i in range(n)])
    poses[:, :3, 3] += 0.02 * np.arange(n)[:, None] * np.array([1.0, 0.5, -0.25], dtype=np.float32)
    want = sequential(hip_device, depth, rgb, scene.K, poses)
    live = LiveFusion(scene.BOUNDS.copy(), voxel_size=scene.VOXEL, max_depth=5.0, batch=4, device=hip_device)
    on_device = [torch.from_numpy(d).to(hip_device).reshape(1, 1, scene.HEIGHT, scene.WIDTH) for d in depth]
    live.add(on_device[0], rgb[0], scene.K, poses[0])          # allocates the rings and the pinned slots
    torch.cuda.synchronize(hip_device)
    torch.cuda.set_sync_debug_mode("error")
    try:
        for i in range(1, n):
            live.add(on_device[i], rgb[i], scene.K, poses[i])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert live._pending == 1 and live.frames == n
    assert not torch.equal(live._volume._weight, want._weight)      # the ninth frame is not in yet
    vol = live.volume
    assert live._pending == 0 and torch.equal(vol._weight, want._weight) and same(vol, want)


def test_live_fusion_on_its_default_device(hip_device):
    """``LiveFusion(bounds)`` is built for "cuda", which names no index; the depth it is given lies on "cuda:0"."""
    from dvmvs.tsdf import LiveFusion
    depth, rgb = scene.frames()
    poses = scene.poses()
    torch.cuda.set_device(hip_device)
    live = LiveFusion(scene.BOUNDS.copy(), voxel_size=scene.VOXEL, batch=2)
    assert live.device == torch.empty(1, device="cuda").device and live.device.index is not None
    for i in (0, 1, 4):
        live.add(torch.from_numpy(depth[i]).to("cuda"), rgb[i], scene.K, poses[i])
    with pytest.raises(ValueError, match="float32 tensor on cuda"):
        live.add(torch.from_numpy(depth[0]), rgb[0], scene.K, poses[0])        # a host depth is still refused
    want = sequential(hip_device, depth[[0, 1, 4]], rgb[[0, 1, 4]], scene.K, poses[[0, 1, 4]])
    assert int((want._weight > 0).sum()) >= 7000 and same(live.volume, want)


def test_live_fusion_takes_the_colour_from_the_device_too(hip_device, six):
    from dvmvs.tsdf import LiveFusion
    depth, rgb, poses, want = six
    live = LiveFusion(scene.BOUNDS.copy(), voxel_size=scene.VOXEL, batch=4, device=hip_device)
    for i in range(6):
        colour = torch.from_numpy(rgb[i]).to(hip_device) if i % 2 else torch.from_numpy(rgb[i])       # device and host tensors in turn
        live.add(torch.from_numpy(depth[i]).to(hip_device), colour, scene.K, poses[i])
    assert same(live.volume, want)


def test_integrate_takes_an_image_that_is_not_row_major(hip_device, six):
    """``resize_nearest(...).astype(uint8)``, the image ``dvmvs.tsdf.run`` integrates, comes out of numpy's indexing with other strides
    than a row-major array's; ``integrate`` fuses what the array holds, not how it lies in memory."""
    from dvmvs.dataset_loader import resize_nearest
    depth, _, poses, _ = six
    rng = np.random.RandomState(5)
    image = resize_nearest(rng.randint(0, 256, (2 * scene.HEIGHT + 1, 2 * scene.WIDTH + 3, 3)).astype(np.float32), scene.WIDTH,
                           scene.HEIGHT).astype(np.uint8)
    transposed = np.ascontiguousarray(image.transpose(1, 0, 2)).transpose(1, 0, 2)       # the same values, certainly not row-major
    assert image.shape == transposed.shape == (scene.HEIGHT, scene.WIDTH, 3) and not transposed.flags["C_CONTIGUOUS"]
    want = fresh(hip_device)
    want.integrate(np.ascontiguousarray(image), depth[0], scene.K, poses[0])
    assert int((want._color > 0).sum()) > 5000
    for layout in (image, transposed):
        got = fresh(hip_device)
        got.integrate(layout, depth[0], scene.K, poses[0])
        assert same(got, want)


# ---- the runners' fuse= hook --------------------------------------------------------------------------------------------------------------
MAX_DEPTH, LIVE_VOXEL = 5.0, 0.1


@pytest.fixture(scope="module")
def run_scene(hip_device, tmp_path_factory):
    from test_runner import _write_scene
    from dvmvs.config import Config
    from dvmvs.engine import DepthEngine
    from dvmvs.fusionnet.model import CostVolumeDecoder, CostVolumeEncoder, FeatureExtractor, FeatureShrinker, LSTMFusion
    from dvmvs.keyframe_buffer import simulate_keyframe_index, write_keyframe_index
    from dvmvs.runner import Scene
    folder = str(tmp_path_factory.mktemp("fuse") / "scene")
    _write_scene(folder, 30)
    sc = Scene(folder)
    lines = simulate_keyframe_index(sc.poses, sc.image_names, Config.test_n_measurement_frames)
    assert len(lines) >= 6
    lines = lines[:3] + ["TRACKING LOST"] + lines[3:]
    index = os.path.join(os.path.dirname(folder), "keyframe+synthetic+scene+nmeas+2")
    write_keyframe_index(index, lines)
    engine = DepthEngine(*syn.build_e2e_modules((FeatureExtractor, FeatureShrinker, CostVolumeEncoder, LSTMFusion, CostVolumeDecoder)),
                         device=hip_device)
    return {"folder": folder, "index": index, "engine": engine, "scene": sc}


def _file_route(hip_device, sc, log, predictions, bounds, width, height):
    """What ``dvmvs.tsdf.run`` would fuse from the saved predictions: per-frame ``integrate`` of the masked predictions with its colours,
    scaled intrinsics and poses."""
    from dvmvs.dataset_loader import PreprocessImage, load_image, resize_nearest
    from dvmvs.tsdf import TSDFVolume
    names = [line.split(" ")[0] for line in log if line != "TRACKING LOST"]
    assert len(names) == len(predictions) > 0
    first = load_image(os.path.join(sc.folder, "images", sc.image_names[0]))
    scaled_K = PreprocessImage(K=sc.K, old_width=first.shape[1], old_height=first.shape[0], new_width=width, new_height=height,
                               distortion_crop=0, perform_crop=False).get_updated_intrinsics()
    vol = TSDFVolume(bounds.copy(), LIVE_VOXEL, device=hip_device)
    for name, prediction in zip(names, predictions):
        image = resize_nearest(load_image(os.path.join(sc.folder, "images", name)), width, height).astype(np.uint8)
        prediction = np.array(prediction, dtype=np.float32)
        prediction[prediction > MAX_DEPTH] = 0.0
        vol.integrate(image, prediction, scaled_K, sc.poses[sc.image_names.index(name)], obs_weight=1.0)
    return vol, scaled_K


def _bounds(sc, width, height):
    from dvmvs.dataset_loader import PreprocessImage
    from dvmvs.tsdf import TSDFFusion
    K = PreprocessImage(K=sc.K, old_width=540, old_height=360, new_width=width, new_height=height, distortion_crop=0,
                        perform_crop=False).get_updated_intrinsics()
    return TSDFFusion.frustum_bounds(list(sc.poses), K, height, width, MAX_DEPTH)


def _check_live_run(hip_device, sc, predict, width=320, height=256):
    """``predict(fuse, frame_log)`` -> predictions.  Runs it with and without ``fuse=``; the live volume equals the file route's."""
    from dvmvs.tsdf import LiveFusion
    bounds = _bounds(sc, width, height)
    live = LiveFusion(bounds, voxel_size=LIVE_VOXEL, max_depth=MAX_DEPTH, batch=4, device=hip_device)
    log = []
    predictions = predict(live, log)
    plain = predict(None, None)
    assert len(predictions) == len(plain) and all(np.array_equal(a, b) for a, b in zip(predictions, plain))
    want, scaled_K = _file_route(hip_device, sc, log, predictions, bounds, width, height)
    assert live.frames == len(predictions)
    assert same(live.volume, want)
    return live, log, scaled_K


@pytest.mark.parametrize("device_evaluate", [False, True])
def test_predict_offline_fuses_what_the_file_route_fuses(hip_device, run_scene, device_evaluate):
    from dvmvs.runner import predict_offline
    sc, engine = run_scene["scene"], run_scene["engine"]

    def predict(fuse, log):
        return predict_offline(engine, run_scene["folder"], run_scene["index"], evaluate=True, max_frames=12, frame_log=log,
                               device_evaluate=device_evaluate, fuse=fuse)[0]

    live, log, scaled_K = _check_live_run(hip_device, sc, predict)
    assert "TRACKING LOST" in log and int((live.volume._weight > 0).sum()) > 0
    # the reconstruction exists when the run ends: the first keyframe's view meets a surface
    first = sc.image_names.index([line for line in log if line != "TRACKING LOST"][0].split(" ")[0])
    depth, _, _ = live.volume.render(scaled_K, sc.poses[first], 256, 320, normals=False, colour=False)
    assert int((depth > 0).sum()) > 0


def test_predict_online_fuses_what_the_file_route_fuses(hip_device, run_scene):
    from dvmvs.runner import predict_online
    sc, engine = run_scene["scene"], run_scene["engine"]

    def predict(fuse, log):
        return predict_online(engine, run_scene["folder"], evaluate=False, max_frames=16, frame_log=log, fuse=fuse)[0]

    live, _, _ = _check_live_run(hip_device, sc, predict)
    assert int((live.volume._weight > 0).sum()) > 0            # not two untouched volumes


def test_predict_mvdepthnet_fuses_what_the_file_route_fuses(hip_device, run_scene):
    from dvmvs.baselines import runner as baselines
    sc = run_scene["scene"]
    with open(run_scene["index"]) as f:
        lines = [line.strip() for line in f if line.strip()][:6]

    def predict(fuse, log):
        if log is not None:
            log.extend(lines)
        return baselines.predict_mvdepthnet(run_scene["folder"], run_scene["index"], evaluate=False, max_frames=6, device=hip_device,
                                            fuse=fuse)[0]

    live, _, _ = _check_live_run(hip_device, sc, predict, baselines.WIDTH, baselines.HEIGHT)
    assert int((live.volume._weight > 0).sum()) > 0            # seeded weights: their depth must still fall inside the volume


def test_predict_sharded_hands_each_scene_its_own_fusion(hip_device, run_scene):
    """The factory is called for the scenes this rank owns, and a scene's volume is the one ``predict_offline`` fuses."""
    from dvmvs.runner import predict_offline, predict_sharded
    from dvmvs.tsdf import LiveFusion
    sc, engine = run_scene["scene"], run_scene["engine"]
    bounds = _bounds(sc, 320, 256)
    made = {}

    def factory(s):
        made[s] = LiveFusion(bounds, voxel_size=LIVE_VOXEL, max_depth=MAX_DEPTH, batch=4, device=hip_device) if s != 2 else None
        return made[s]

    folders, indices = [run_scene["folder"]] * 3, [run_scene["index"]] * 3
    results, _ = predict_sharded(lambda: engine, folders, indices, evaluate=False, max_frames=8, rank=0, world=2, fuse=factory)
    assert sorted(results) == [0, 2] and sorted(made) == [0, 2] and made[2] is None       # scene 1 is another rank's
    want = LiveFusion(bounds, voxel_size=LIVE_VOXEL, max_depth=MAX_DEPTH, batch=4, device=hip_device)
    plain = predict_offline(engine, run_scene["folder"], run_scene["index"], evaluate=False, max_frames=8, fuse=want)[0]
    assert made[0].frames == len(plain) == len(results[0][0]) > 0
    assert int((want.volume._weight > 0).sum()) > 0 and same(made[0].volume, want.volume)


def test_the_fuse_flag_of_the_baselines_writes_the_live_mesh(hip_device, run_scene, tmp_path, capsys):
    """``python -m dvmvs.baselines.mvdepthnet ... --fuse``: a LiveFusion on the default device, sized from the scene's poses alone, and
    the mesh of its volume next to the results."""
    from dvmvs.baselines import runner as baselines
    from dvmvs.tsdf import LiveFusion
    torch.cuda.set_device(hip_device)
    live = baselines.live_fusion_for_scene(run_scene["folder"], (baselines.WIDTH, baselines.HEIGHT), 0.1, MAX_DEPTH, 4)
    assert isinstance(live, LiveFusion) and live.batch == 4 and live.max_depth == MAX_DEPTH
    out = str(tmp_path / "results")
    os.makedirs(out)
    baselines.main("mvdepthnet", [run_scene["folder"], run_scene["index"], "--out", out, "--max-frames", "6", "--fuse",
                                  "--fuse_voxel_size", "0.1", "--fuse_max_depth", str(MAX_DEPTH), "--fuse_batch", "4"])
    capsys.readouterr()
    name = baselines.system_name("mvdepthnet", run_scene["index"])
    mesh = os.path.join(out, f"{name}_scene_live_complete.ply")
    assert os.path.exists(mesh)
    with open(mesh) as f:
        header = [next(f).strip() for _ in range(3)]
    assert header[:2] == ["ply", "format ascii 1.0"] and int(header[2].split()[-1]) > 0        # "element vertex N": a surface was fused

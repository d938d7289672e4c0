"""GPU: the frame pre-processing kernels (csrc/preprocess.hip) on every launch path -- 16-byte and scalar stores, padded source rows,
strided and misaligned destinations, N in {1, 4}, both normalisations and none -- against the float64 reference of
tests/preprocess_reference.py (pinned on the CPU by tests/test_preprocess_reference.py) within the derived rounding bound, bit for bit
against the host functions, through the public surface, and through the scene runners in both modes."""
import os

import numpy as np
import pytest
import torch

import preprocess_reference as ref
import synthetic as syn

pytestmark = pytest.mark.gpu

NORMALISATIONS = {"imagenet": ref.IMAGENET + (True,), "baseline": ref.BASELINE + (True,), "raw": ref.BASELINE + (False,)}


@pytest.fixture(scope="module")
def ops():
    from dvmvs.hip import ops
    return ops


def _frames(kind, N, H, W, golden_dir):
    if kind == "random":
        return ref.random_frames(N, H, W, seed=21)
    if kind == "spikes":
        return ref.spike_frames(N, H, W, seed=22)
    from dvmvs.dataset_loader import load_image_u8
    image = load_image_u8(os.path.join(golden_dir, "sample_scene", "images", "00012.png"))
    other = load_image_u8(os.path.join(golden_dir, "sample_scene", "images", "00013.png"))
    assert image.shape == (H, W, 3)
    return np.stack([image, other, image[::-1], other[:, ::-1]][:N])


def _host_rgb(frames, case, scale, mean, std, normalize):
    H, W, new_h, new_w, crop_x, crop_y = ref.CASES[case]
    pre = ref.preprocessor(H, W, new_h, new_w, crop_x, crop_y)
    return np.stack([np.transpose(pre.apply_rgb(f.astype(np.float32), scale, list(mean), list(std), normalize_colors=normalize), (2, 0, 1))
                     for f in frames])


def _check_rgb(got, frames, case, norm, what):
    """Every element: within the derived bound of the float64 reference, and equal to the host function bit for bit."""
    H, W, new_h, new_w, crop_x, crop_y = ref.CASES[case]
    scale, mean, std, normalize = NORMALISATIONS[norm]
    got = got.cpu().numpy()
    want = ref.preprocess_rgb(frames, crop_x, crop_y, new_h, new_w, scale, mean, std, normalize)
    assert got.shape == want.shape and got.dtype == np.float32
    bound = ref.tolerance(scale, mean, std, normalize)
    err = float(np.max(np.abs(got.astype(np.float64) - want)))
    host = _host_rgb(frames, case, scale, mean, std, normalize)
    differing = int(np.count_nonzero(got != host))
    print(f"{what} {case} {norm}: max|kernel - float64| {err:.3e} (bound {bound:.3e}); elements differing from the host path {differing}")
    assert np.isfinite(got).all() and err <= bound, (what, case, norm, err, bound)
    assert differing == 0, (what, case, norm, differing, float(np.max(np.abs(got - host))))


@pytest.mark.parametrize("norm", sorted(NORMALISATIONS))
@pytest.mark.parametrize("case", sorted(ref.CASES))
def test_preprocess_rgb_on_every_shape(ops, hip_device, golden_dir, case, norm):
    """Random and isolated 0 / 255 frames (N = 4) and, at its size, the real sample frame (N = 1 and 4)."""
    H, W, new_h, new_w, crop_x, crop_y = ref.CASES[case]
    scale, mean, std, normalize = NORMALISATIONS[norm]
    kinds = [("random", 4), ("spikes", 4), ("random", 1)] + ([("real", 1), ("real", 4)] if (H, W) == (360, 540) else [])
    for kind, N in kinds:
        frames = _frames(kind, N, H, W, golden_dir)
        got = ops.preprocess_rgb(torch.from_numpy(frames).to(hip_device), crop_x, crop_y, new_h, new_w, scale, mean, std, normalize=normalize)
        assert tuple(got.shape) == (N, 3, new_h, new_w)
        _check_rgb(got, frames, case, norm, f"{kind} N={N}")


def test_identity_size_without_normalisation_returns_the_pixels(ops, hip_device):
    frames = ref.random_frames(4, 240, 320, seed=5)
    got = ops.preprocess_rgb(torch.from_numpy(frames).to(hip_device), 0, 0, 240, 320, 1.0, [0.0] * 3, [1.0] * 3, normalize=False)
    assert np.array_equal(got.cpu().numpy(), np.transpose(frames, (0, 3, 1, 2)).astype(np.float32))
    single = ops.preprocess_rgb(torch.from_numpy(frames[0]).to(hip_device), 0, 0, 240, 320, 1.0, None, None, normalize=False)
    assert tuple(single.shape) == (1, 3, 240, 320) and np.array_equal(single.cpu().numpy()[0], np.transpose(frames[0], (2, 0, 1)))


@pytest.mark.parametrize("case", ["sample_crop", "ragged_odd", "ragged_even", "magnify"])
@pytest.mark.parametrize("N", [1, 4])
def test_padded_source_rows(ops, hip_device, case, N):
    """Rows 3 W + 13 bytes apart (a view into a wider buffer, not copied by the op)."""
    H, W, new_h, new_w, crop_x, crop_y = ref.CASES[case]
    frames = ref.random_frames(N, H, W, seed=31)
    wide = torch.full((N, H, 3 * W + 13), 77, dtype=torch.uint8, device=hip_device)
    view = torch.as_strided(wide, (N, H, W, 3), (H * (3 * W + 13), 3 * W + 13, 3, 1))
    view.copy_(torch.from_numpy(frames))
    assert view.stride(1) == 3 * W + 13 and view.data_ptr() == wide.data_ptr()
    for norm in ("imagenet", "raw"):
        scale, mean, std, normalize = NORMALISATIONS[norm]
        got = ops.preprocess_rgb(view, crop_x, crop_y, new_h, new_w, scale, mean, std, normalize=normalize)
        _check_rgb(got, frames, case, norm, f"padded rows N={N}")


@pytest.mark.parametrize("case", ["sample_nocrop", "ragged_odd", "ragged_even"])
@pytest.mark.parametrize("offset", [0, 4, 1, 3])
def test_strided_and_misaligned_destinations(ops, hip_device, case, offset):
    """``out`` = a slot of a larger buffer: batch stride larger than a frame, start ``offset`` floats past a 16-byte boundary (0 and 4 keep
    the 16-byte store path where the width allows it, 1 and 3 force the scalar one); nothing outside the slots is written."""
    H, W, new_h, new_w, crop_x, crop_y = ref.CASES[case]
    N, frame = 4, 3 * new_h * new_w
    frames = ref.random_frames(N, H, W, seed=41)
    raw = torch.from_numpy(frames).to(hip_device)
    for stride in (frame + 8, frame + 5):
        canary = -12345.0
        buffer = torch.full((offset + N * stride + 16,), canary, dtype=torch.float32, device=hip_device)
        assert buffer.data_ptr() % 16 == 0
        out = torch.as_strided(buffer, (N, 3, new_h, new_w), (stride, new_h * new_w, new_w, 1), offset)
        got = ops.preprocess_rgb(raw, crop_x, crop_y, new_h, new_w, *NORMALISATIONS["baseline"][:3], out=out)
        assert got.data_ptr() == out.data_ptr()
        _check_rgb(out, frames, case, "baseline", f"offset {offset} stride {stride}")
        written = torch.zeros_like(buffer, dtype=torch.bool)
        torch.as_strided(written, (N, frame), (stride, 1), offset).fill_(True)
        assert bool((buffer[~written] == canary).all())


@pytest.mark.parametrize("case", sorted(ref.CASES))
@pytest.mark.parametrize("N", [1, 4])
def test_preprocess_depth_equals_the_host_path(ops, hip_device, case, N):
    """Equality with apply_depth(depth as float64 / scaling).astype(float32), values 0 and 65535 included; uint16 and int16 carriers."""
    H, W, new_h, new_w, crop_x, crop_y = ref.CASES[case]
    depth = ref.random_depths(N, H, W, seed=51)
    pre = ref.preprocessor(H, W, new_h, new_w, crop_x, crop_y)
    for scaling in (1000.0, 5000.0):
        want = np.stack([pre.apply_depth(d.astype(np.float64) / scaling).astype(np.float32) for d in depth])
        got = ops.preprocess_depth(torch.from_numpy(depth.view(np.int16)).to(hip_device), crop_x, crop_y, new_h, new_w, scaling=scaling)
        assert tuple(got.shape) == (N, new_h, new_w) and np.array_equal(got.cpu().numpy(), want)
        assert want.max() == np.float32(65535 / scaling) and want.min() == 0.0
        assert np.array_equal(want, ref.preprocess_depth(depth, crop_x, crop_y, new_h, new_w, scaling).astype(np.float32))
    want = np.stack([pre.apply_depth(d.astype(np.float64) / 1000.0).astype(np.float32) for d in depth])
    if hasattr(torch, "uint16"):
        out = torch.empty((N, new_h, new_w), dtype=torch.float32, device=hip_device)
        got = ops.preprocess_depth(torch.from_numpy(depth).to(hip_device), crop_x, crop_y, new_h, new_w, out=out)
        assert got.data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy(), want)
    # a destination that is not 16-byte aligned takes the scalar stores
    buffer = torch.zeros((N * new_h * new_w + 4,), dtype=torch.float32, device=hip_device)
    out = buffer[1:1 + N * new_h * new_w].view(N, new_h, new_w)
    ops.preprocess_depth(torch.from_numpy(depth.view(np.int16)).to(hip_device), crop_x, crop_y, new_h, new_w, out=out)
    assert np.array_equal(out.cpu().numpy(), want) and float(buffer[0]) == 0.0 and bool((buffer[-3:] == 0).all())


def test_ops_refuse_bad_arguments(ops, hip_device):
    raw = torch.zeros((2, 8, 12, 3), dtype=torch.uint8, device=hip_device)
    args = (255.0, [0.5] * 3, [0.5] * 3)
    with pytest.raises(TypeError):
        ops.preprocess_rgb(raw.float(), 0, 0, 4, 6, *args)
    with pytest.raises(ValueError):
        ops.preprocess_rgb(raw[..., :2], 0, 0, 4, 6, *args)
    with pytest.raises(ValueError):
        ops.preprocess_rgb(raw, 6, 0, 4, 6, *args)                       # the crop leaves no columns
    with pytest.raises(ValueError):
        ops.preprocess_rgb(raw, 0, 0, 4, 6, 255.0, [0.5] * 3, [0.5, 0.0, 0.5])
    with pytest.raises(ValueError):
        ops.preprocess_rgb(raw, 0, 0, 4, 6, *args, out=torch.empty((2, 3, 4, 7), device=hip_device))
    with pytest.raises(ValueError):
        ops.preprocess_rgb(raw, 0, 0, 4, 6, *args, out=torch.empty((2, 4, 6, 3), device=hip_device).permute(0, 3, 1, 2))
    with pytest.raises(TypeError):
        ops.preprocess_depth(torch.zeros((8, 12), dtype=torch.int32, device=hip_device), 0, 0, 4, 6)
    with pytest.raises(ValueError):
        ops.preprocess_depth(torch.zeros((8, 12), dtype=torch.int16, device=hip_device), 0, 0, 4, 6, scaling=0.0)


def test_public_surface(hip_device, golden_dir):
    """PreprocessImage.apply_rgb_device / apply_depth_device: numpy, host tensor, device tensor and uploader inputs, ``out=`` honoured,
    the crop the constructor derives (540x360 -> 320x256: 45 columns)."""
    from dvmvs.dataset_loader import FrameUploader, PreprocessImage, load_depth_png, load_depth_png_u16, load_image, load_image_u8
    K = np.loadtxt(os.path.join(golden_dir, "hololens_000_K.txt"))
    image_path = os.path.join(golden_dir, "sample_scene", "images", "00012.png")
    depth_path = os.path.join(golden_dir, "sample_scene", "depth", "00012.png")
    u8, u16 = load_image_u8(image_path), load_depth_png_u16(depth_path)
    uploader = FrameUploader(hip_device, slots=2)
    for crop in (True, False):
        pre = PreprocessImage(K, 540, 360, 320, 256, distortion_crop=0, perform_crop=crop)
        assert pre.crop_x == (45 if crop else 0)
        case = "sample_crop" if crop else "sample_nocrop"
        for norm in ("imagenet", "baseline", "raw"):
            scale, mean, std, normalize = NORMALISATIONS[norm]
            host = np.transpose(pre.apply_rgb(load_image(image_path), scale, list(mean), list(std), normalize_colors=normalize), (2, 0, 1))[None]
            inputs = {"numpy": dict(image_u8=u8, device=hip_device), "host tensor": dict(image_u8=torch.from_numpy(u8.copy()), device=hip_device),
                      "device tensor": dict(image_u8=torch.from_numpy(u8.copy()).to(hip_device)),
                      "uploader": dict(image_u8=u8, device=hip_device, uploader=uploader)}
            for what, kwargs in inputs.items():
                got = pre.apply_rgb_device(scale_rgb=scale, mean_rgb=list(mean), std_rgb=list(std), normalize_colors=normalize, **kwargs)
                assert got.device == hip_device and tuple(got.shape) == (1, 3, 256, 320)
                _check_rgb(got, u8[None], case, norm, f"apply_rgb_device({what})")
                assert np.array_equal(got.cpu().numpy(), host)
        batch = np.stack([u8, u8[::-1]])
        slot = torch.zeros((2, 2, 3, 256, 320), dtype=torch.float32, device=hip_device)
        got = pre.apply_rgb_device(batch, *ref.IMAGENET, device=hip_device, out=slot[:, 1])
        assert got.data_ptr() == slot[:, 1].data_ptr() and float(slot[:, 0].abs().max()) == 0.0
        _check_rgb(slot[:, 1], batch, case, "imagenet", "apply_rgb_device(out=)")
        want = pre.apply_depth(load_depth_png(depth_path)).astype(np.float32)
        for what, kwargs in {"numpy": dict(depth_u16=u16, device=hip_device), "uploader": dict(depth_u16=u16, device=hip_device, uploader=uploader),
                             "device tensor": dict(depth_u16=torch.from_numpy(u16.view(np.int16).copy()).to(hip_device))}.items():
            got = pre.apply_depth_device(**kwargs)
            assert tuple(got.shape) == (1, 256, 320) and np.array_equal(got.cpu().numpy()[0], want), what
    # the ring on the device: more uploads than slots, every result intact
    frames = ref.random_frames(7, 48, 64, seed=61)
    on_device = [uploader.upload_rgb(f) for f in frames]
    torch.cuda.synchronize()
    assert all(np.array_equal(d.cpu().numpy(), f) for d, f in zip(on_device, frames))
    assert all(b.is_pinned() for b in uploader._buffers)


def test_a_batch_is_one_launch(hip_device):
    """apply_rgb_device of a [4,H,W,3] batch on the device is ONE kernel (crop, resize, normalisation and transposition included)."""
    from torch.profiler import ProfilerActivity, profile
    pre = ref.preprocessor(*ref.CASES["sample_crop"])
    raw = torch.from_numpy(ref.random_frames(4, 360, 540, seed=71)).to(hip_device)
    out = torch.empty((4, 3, 256, 320), dtype=torch.float32, device=hip_device)
    pre.apply_rgb_device(raw, *ref.IMAGENET, out=out)           # library load, first-launch set-up
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        pre.apply_rgb_device(raw, *ref.IMAGENET, out=out)
        torch.cuda.synchronize()
    activity = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]      # kernels, copies, memsets: everything
    print("device activity:", activity)
    assert len(activity) == 1 and "preprocess_rgb_kernel" in activity[0], activity


# ---- runners: device_preprocess=True against the host path ----------------------------------------------------------------------------
def _engine(hip_device):
    from dvmvs.engine import DepthEngine
    from dvmvs.fusionnet.model import CostVolumeDecoder, CostVolumeEncoder, FeatureExtractor, FeatureShrinker, LSTMFusion
    return DepthEngine(*syn.build_e2e_modules((FeatureExtractor, FeatureShrinker, CostVolumeEncoder, LSTMFusion, CostVolumeDecoder)),
                       device=hip_device)


def _compare_modes(run, what):
    """The kernel reproduces the host path bit for bit (asserted above on every shape), so the two modes feed the network identical
    inputs: identical predictions, frame logs and -- after the host's float64 is cast -- ground-truth depths.  Each mode gets a fresh
    engine / network so that both go through the same sequence of eager and replayed frames."""
    log_host, log_device = [], []
    preds_host, gts_host = run(False, log_host)
    preds_device, gts_device = run(True, log_device)
    assert log_host == log_device and len(preds_host) == len(preds_device) >= 2
    worst = max(float(np.max(np.abs(a - b))) for a, b in zip(preds_host, preds_device))
    print(f"{what}: {len(preds_host)} predictions, max |device mode - host mode| {worst:.3e}")
    assert all(np.array_equal(a, b) for a, b in zip(preds_host, preds_device))
    if gts_host is not None:
        assert len(gts_host) == len(gts_device) == len(preds_host)
        assert all(b.dtype == np.float32 and np.array_equal(a.astype(np.float32), b) for a, b in zip(gts_host, gts_device))


def test_predict_offline_in_both_modes(hip_device, tmp_path):
    from test_runner import _write_scene
    from dvmvs.runner import predict_offline
    scene = os.path.join(str(tmp_path), "scene")
    _write_scene(scene, 24)
    index = os.path.join(str(tmp_path), "index")
    with open(index, "w") as f:
        f.write("00009.png 00006.png 00003.png\n00010.png 00009.png 00006.png\nTRACKING LOST\n00013.png 00010.png 00009.png\n")

    def run(device_preprocess, log):
        preds, gts, _ = predict_offline(_engine(hip_device), scene, index, evaluate=True, frame_log=log, device_preprocess=device_preprocess)
        return preds, gts

    _compare_modes(run, "predict_offline")


def test_predict_online_in_both_modes(hip_device, tmp_path):
    from test_runner import _write_scene
    from dvmvs.runner import predict_online
    scene = os.path.join(str(tmp_path), "scene")
    _write_scene(scene, 24)

    def run(device_preprocess, log):
        preds, gts, _ = predict_online(_engine(hip_device), scene, evaluate=True, max_frames=16, frame_log=log,
                                       device_preprocess=device_preprocess)
        return preds, gts

    _compare_modes(run, "predict_online")


def test_predict_mvdepthnet_in_both_modes(hip_device, tmp_path):
    from test_baselines_gpu import _write_scene
    from dvmvs.baselines import runner
    index = _write_scene(str(tmp_path / "scene"))

    def run(device_preprocess, log):
        preds, gts, _ = runner.predict_mvdepthnet(str(tmp_path / "scene"), index, device=hip_device, device_preprocess=device_preprocess)
        return preds, gts

    _compare_modes(run, "predict_mvdepthnet")


def test_baseline_command_line_switch(hip_device, tmp_path):
    """``python -m dvmvs.baselines.mvdepthnet ... --device-preprocess`` writes the predictions the default writes."""
    from test_baselines_gpu import _write_scene
    from dvmvs.baselines import runner
    index = _write_scene(str(tmp_path / "scene"))
    saved = []
    for flag in ([], ["--device-preprocess"]):
        out = tmp_path / ("out" + str(len(flag)))
        out.mkdir()
        runner.main("mvdepthnet", [str(tmp_path / "scene"), index, "--out", str(out)] + flag)
        name = runner.system_name("mvdepthnet", index)
        saved.append(np.load(out / f"{name}_predictions_000.npz")["arr_0"])
    assert saved[0].shape == (2, 256, 320) and np.array_equal(saved[0], saved[1])


def test_tsdf_switch_writes_the_same_meshes(hip_device, golden_dir, tmp_path):
    """``dvmvs.tsdf.run(device_preprocess=True)`` (8-bit image loading) against the default: the .ply files are equal byte for byte.
    Scene as in tests/test_marching_cubes_gpu.py: two keyframes of the sample scene, their depth maps as 'predictions'."""
    from PIL import Image
    from dvmvs.dataset_loader import load_depth_png, resize_nearest
    from dvmvs.tsdf import main
    src = os.path.join(golden_dir, "sample_scene")
    scene = tmp_path / "data" / "hololens-dataset" / "000"
    (scene / "images").mkdir(parents=True)
    (scene / "depth").mkdir()
    names = ["00012.png", "00013.png"]
    for name in names:
        Image.open(os.path.join(src, "images", name)).save(scene / "images" / name)
        Image.open(os.path.join(src, "depth", name)).save(scene / "depth" / name)
    np.savetxt(scene / "poses.txt", np.loadtxt(os.path.join(golden_dir, "hololens_000_poses.txt")).reshape(-1, 16)[[9, 10]])
    np.savetxt(scene / "K.txt", np.loadtxt(os.path.join(golden_dir, "hololens_000_K.txt")))
    (tmp_path / "data" / "indices").mkdir()
    (tmp_path / "data" / "indices" / "keyframe+hololens-dataset+000+nmeas+3").write_text("00012.png 00009.png\nTRACKING LOST\n00013.png 00012.png\n")
    preds = np.stack([resize_nearest(load_depth_png(os.path.join(src, "depth", n)), 320, 256) for n in names]).astype(np.float32)
    (tmp_path / "pred").mkdir()
    np.savez(tmp_path / "pred" / "keyframe_hololens-dataset_320_256_3_dvmvs_fusionnet_online_predictions_000.npz", preds)
    meshes = []
    for tag, flag in (("host", []), ("device", ["--device-preprocess"])):
        out = tmp_path / tag
        main(["--reconstruction_folder", str(out), "--prediction_folder", str(tmp_path / "pred"), "--data_folder", str(tmp_path / "data"),
              "--voxel_size", "0.05", "--save_groundtruth"] + flag)
        written = sorted(os.listdir(out))
        assert len(written) == 2
        meshes.append([(w, open(out / w, "rb").read()) for w in written])
    assert meshes[0] == meshes[1] and all(len(data) > 10000 for _, data in meshes[0])

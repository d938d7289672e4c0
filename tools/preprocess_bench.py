"""Frame pre-processing, host path against device path, on the GPU box: writes profiles/preprocess_bench.json.

For a 540x360 and a 640x480 8-bit frame -> 320x256 (the crop PreprocessImage derives, ImageNet normalisation):
  host    per image, as the runners' default path does it: PreprocessImage.apply_rgb (numpy) + transpose + blocking .to(device), synchronised
  device  per image: FrameUploader.upload_rgb (pinned ring, non-blocking copy) + dvmvs::preprocess_rgb, synchronised
  kernel  the kernel alone, from `rocprofv3 --kernel-trace --stats` over a child process of this tool (--kernel-loop); the CSV is
          copied to profiles/preprocess_kernel_stats.csv
The per-image figures are synchronised, unpipelined latencies (the two paths alternate, each waits for the device before the next
starts, so the ring is never more than one slot deep): what one image costs, not what a pipelined loader sustains.
Then predict_offline over a synthetic 24-frame scene in both modes (wall clock around the call, frames per second; the PNG decoding both
modes share is timed separately).

    python tools/preprocess_bench.py [--images 300] [--warmup 30] [--out profiles] [--no-rocprof]
"""
import argparse
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
for _p in (os.path.join(ROOT, "deep-video-mvs_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SIZES = {"540x360": (360, 540), "640x480": (480, 640)}
KERNEL_LOOP_LAUNCHES = 500


def _preprocessor(H, W):
    from dvmvs.config import Config
    from dvmvs.dataset_loader import PreprocessImage
    return PreprocessImage(K=np.eye(3), old_width=W, old_height=H, new_width=Config.test_image_width, new_height=Config.test_image_height,
                           distortion_crop=Config.test_distortion_crop, perform_crop=Config.test_perform_crop)


def _stats(seconds):
    ms = np.asarray(seconds) * 1e3
    return {"median_ms": float(np.median(ms)), "p90_ms": float(np.percentile(ms, 90)), "min_ms": float(ms.min()), "images": int(ms.size)}


def per_image(H, W, images, warmup, device):
    from dvmvs.dataset_loader import FrameUploader
    from dvmvs.runner import MEAN_RGB, SCALE_RGB, STD_RGB, _to_device
    pre = _preprocessor(H, W)
    rng = np.random.RandomState(0)
    frames_u8 = [rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8) for _ in range(8)]
    frames_f32 = [f.astype(np.float32) for f in frames_u8]      # load_image returns float32: the conversion is part of decoding
    uploader = FrameUploader(device)
    host, dev = [], []
    for k in range(warmup + images):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a = _to_device(pre.apply_rgb(frames_f32[k % 8], SCALE_RGB, MEAN_RGB, STD_RGB), device)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        b = pre.apply_rgb_device(frames_u8[k % 8], SCALE_RGB, MEAN_RGB, STD_RGB, device=device, uploader=uploader)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if k >= warmup:
            host.append(t1 - t0)
            dev.append(t2 - t1)
    equal = bool(torch.equal(a, b))
    return {"host": _stats(host), "device": _stats(dev), "host_over_device_median": float(np.median(host) / np.median(dev)),
            "crop": [pre.crop_x, pre.crop_y], "last_image_bit_identical": equal}


def kernel_loop(device):
    """Child process under rocprofv3: the kernel alone, both sizes, KERNEL_LOOP_LAUNCHES launches each."""
    from dvmvs.runner import MEAN_RGB, SCALE_RGB, STD_RGB
    for H, W in SIZES.values():
        pre = _preprocessor(H, W)
        raw = torch.randint(0, 256, (1, H, W, 3), dtype=torch.uint8, device=device)
        out = torch.empty((1, 3, pre.new_height, pre.new_width), dtype=torch.float32, device=device)
        for _ in range(KERNEL_LOOP_LAUNCHES):
            pre.apply_rgb_device(raw, SCALE_RGB, MEAN_RGB, STD_RGB, out=out)
        torch.cuda.synchronize()


def kernel_alone(out_dir):
    """Runs `rocprofv3 --kernel-trace --stats` over a fresh child and returns the preprocess kernels' rows of its kernel_stats CSV."""
    import csv
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        return {"error": "rocprofv3 not found"}
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [rocprof, "--kernel-trace", "--stats", "-d", tmp, "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
               "--kernel-loop"]
        done = subprocess.run(cmd, cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if done.returncode != 0 or not files:
            return {"error": f"rocprofv3 exit {done.returncode}", "log_tail": done.stdout[-600:]}
        rows = [r for r in csv.DictReader(open(files[0])) if "preprocess" in r.get("Name", "")]
        shutil.copy(files[0], os.path.join(out_dir, "preprocess_kernel_stats.csv"))
    return {"launches_per_size": KERNEL_LOOP_LAUNCHES, "csv": "profiles/preprocess_kernel_stats.csv",
            "kernels": [{"name": r["Name"].split("(")[0], "calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) / 1e3,
                         "min_us": float(r["MinNs"]) / 1e3, "max_us": float(r["MaxNs"]) / 1e3} for r in rows]}


def _write_scene(folder, n_frames):
    """A synthetic scene folder: smooth-noise 540x360 frames, depth maps, the sample poses (tests/synthetic.py: the helpers shared with
    the tests)."""
    from PIL import Image
    import synthetic as syn
    os.makedirs(os.path.join(folder, "images"))
    os.makedirs(os.path.join(folder, "depth"))
    np.savetxt(os.path.join(folder, "poses.txt"), syn.sample_poses()[:n_frames].reshape(n_frames, 16))
    np.savetxt(os.path.join(folder, "K.txt"), np.loadtxt(os.path.join(syn.GOLDEN_DIR, "hololens_000_K.txt")))
    rng = np.random.RandomState(1)
    for i in range(n_frames):
        img = (syn.smooth_noise((3, 360, 540), seed=600 + i).permute(1, 2, 0).numpy() * 40 + 128).clip(0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(folder, "images", f"{i:05d}.png"))
        Image.fromarray((1500 + 200 * rng.rand(360, 540)).astype(np.uint16)).save(os.path.join(folder, "depth", f"{i:05d}.png"))


def scene_throughput(device, repeats=3):
    import synthetic as syn
    from dvmvs.config import Config
    from dvmvs.dataset_loader import load_image, load_image_u8
    from dvmvs.engine import DepthEngine
    from dvmvs.fusionnet.model import CostVolumeDecoder, CostVolumeEncoder, FeatureExtractor, FeatureShrinker, LSTMFusion
    from dvmvs.keyframe_buffer import simulate_keyframe_index, write_keyframe_index
    from dvmvs.runner import Scene, predict_offline
    result = {}
    with tempfile.TemporaryDirectory() as tmp:
        folder = os.path.join(tmp, "scene")
        _write_scene(folder, 24)
        scene = Scene(folder)
        lines = simulate_keyframe_index(scene.poses, scene.image_names, Config.test_n_measurement_frames)
        index = os.path.join(tmp, "index")
        write_keyframe_index(index, lines)
        paths = [os.path.join(folder, "images", n) for n in scene.image_names]
        for name, loader in (("float32", load_image), ("uint8", load_image_u8)):
            t0 = time.perf_counter()
            for _ in range(3):
                for p in paths:
                    loader(p)
            result[f"png_decode_ms_per_image_{name}"] = (time.perf_counter() - t0) / (3 * len(paths)) * 1e3
        engine = DepthEngine(*syn.build_e2e_modules((FeatureExtractor, FeatureShrinker, CostVolumeEncoder, LSTMFusion, CostVolumeDecoder)),
                             device=device)
        for mode in (False, True):                                  # warm-up: graph capture, MIOpen find
            predict_offline(engine, folder, index, evaluate=False, device_preprocess=mode)
        for mode in (False, True):
            best = None
            for _ in range(repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                preds, _, timer = predict_offline(engine, folder, index, evaluate=False, device_preprocess=mode)
                torch.cuda.synchronize()
                seconds = time.perf_counter() - t0
                best = seconds if best is None else min(best, seconds)
            result["device_preprocess" if mode else "host_preprocess"] = {
                "frames": len(preds), "seconds_best_of_%d" % repeats: best, "frames_per_s": len(preds) / best}
        result["index_lines"] = len(lines)
    return result


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--images", type=int, default=300)
    parser.add_argument("--warmup", type=int, default=30)
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    parser.add_argument("--no-rocprof", action="store_true")
    parser.add_argument("--no-scene", action="store_true")
    parser.add_argument("--kernel-loop", action="store_true", help="(internal) the child process that rocprofv3 traces")
    args = parser.parse_args(argv)
    device = torch.device("cuda:0")
    if args.kernel_loop:
        kernel_loop(device)
        return
    os.makedirs(args.out, exist_ok=True)
    result = {"tool": "tools/preprocess_bench.py", "device": torch.cuda.get_device_name(0), "cpu_threads": torch.get_num_threads(),
              "target": "320x256, ImageNet normalisation", "per_image": {}}
    for name, (H, W) in SIZES.items():
        result["per_image"][name] = per_image(H, W, args.images, args.warmup, device)
    if not args.no_rocprof:
        result["kernel_alone"] = kernel_alone(args.out)
    if not args.no_scene:
        result["predict_offline_24_frame_scene"] = scene_throughput(device)
    with open(os.path.join(args.out, "preprocess_bench.json"), "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()

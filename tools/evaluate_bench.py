"""Depth evaluation on the device, on the GPU box: writes profiles/evaluate_bench.json.

  kernel   dvmvs::depth_errors on 256x320 frames at N = 1 and N = 64, by HIP events: after a warm-up, `--repeats` windows of
           `--launches` back-to-back launches each, the window's time over its launches; the median window is reported.  Each figure is
           taken twice: "graph" = the launches captured once into a hipGraph and the replay timed (no Python, no ctypes between the
           launches: the device's rate, the figure to hold against the launch floor), and "python" = the same launches issued by
           ops.depth_errors calls (what a Python caller pays per call, host issue rate included).  At N = 64 the
           launches rotate over 8 input sets (8 x 42 MB, more than the chip's 256 MB last-level cache), so the figure is a read from HBM,
           and the same loop over ONE input set is reported next to it (cache-resident).  Bytes = 8 per pixel; the share of HBM bandwidth
           is bytes / time over the 8 TB/s peak.
  runner   predict_offline frames per second over a synthetic 24-frame scene with device_preprocess=True, device_evaluate off (every
           frame fetched and evaluated by numpy afterwards: compute_errors is inside the timed region, as save_results would run it) and
           on, in this process, alternating, median of `--scene-repeats` runs; the host-evaluation time alone is listed as well.

    python tools/evaluate_bench.py [--launches 200] [--repeats 30] [--scene-repeats 7] [--out profiles] [--no-scene]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
for _p in (os.path.join(ROOT, "deep-video-mvs_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HEIGHT, WIDTH = 256, 320
HBM_PEAK_BYTES_PER_S = 8.0e12


def _inputs(N, sets, device):
    generator = torch.Generator(device=device).manual_seed(0)
    out = []
    for _ in range(sets):
        gt = torch.rand((N, HEIGHT, WIDTH), device=device, generator=generator) * 6.0
        gt[gt < 1.2] = 0.0
        pred = gt * torch.exp(0.2 * torch.randn((N, HEIGHT, WIDTH), device=device, generator=generator)) + 0.05
        out.append((gt, pred))
    return out


def kernel_time(N, sets, launches, repeats, device):
    from dvmvs.hip import ops
    inputs = _inputs(N, sets, device)
    out = torch.empty((N, 8), dtype=torch.float32, device=device)
    for k in range(3 * sets):
        ops.depth_errors(*inputs[k % sets], out=out)
    torch.cuda.synchronize()

    def issue():
        for k in range(launches):
            ops.depth_errors(*inputs[k % sets], out=out)

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        issue()
    graph.replay()
    torch.cuda.synchronize()
    nbytes = 8 * N * HEIGHT * WIDTH
    result = {"frames": N, "input_sets": sets, "launches_per_window": launches, "windows": repeats, "bytes_read": nbytes}
    for name, run in (("graph", graph.replay), ("python", issue)):
        windows = []
        for _ in range(repeats):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            run()
            end.record()
            end.synchronize()
            windows.append(start.elapsed_time(end) * 1e3 / launches)
        us = float(np.median(windows))
        result[name] = {"median_us_per_launch": us, "min_us_per_launch": float(np.min(windows)), "max_us_per_launch": float(np.max(windows)),
                        "bytes_per_s": nbytes / (us * 1e-6), "share_of_8TBps_hbm_peak": nbytes / (us * 1e-6) / HBM_PEAK_BYTES_PER_S}
    return result


def scene_throughput(device, repeats):
    import synthetic as syn
    from preprocess_bench import _write_scene
    from dvmvs.config import Config
    from dvmvs.engine import DepthEngine
    from dvmvs.errors import compute_errors
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
        engine = DepthEngine(*syn.build_e2e_modules((FeatureExtractor, FeatureShrinker, CostVolumeEncoder, LSTMFusion, CostVolumeDecoder)),
                             device=device)

        def run(device_evaluate):
            rows = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            preds, gts, timer = predict_offline(engine, folder, index, evaluate=True, device_preprocess=True, device_evaluate=device_evaluate,
                                                error_log=rows)
            t1 = time.perf_counter()
            if not device_evaluate:
                rows = [compute_errors(g, p) for g, p in zip(gts, preds)]
            t2 = time.perf_counter()
            return len(preds), t2 - t0, t2 - t1, float(np.median(timer.times))

        for mode in (False, True):                                  # warm-up: graph capture, MIOpen find, workspaces
            run(mode)
        runs = {False: [], True: []}
        for _ in range(repeats):
            for mode in (False, True):
                runs[mode].append(run(mode))
        for mode, name in ((False, "host_evaluate"), (True, "device_evaluate")):
            frames = runs[mode][0][0]
            seconds = float(np.median([r[1] for r in runs[mode]]))
            result[name] = {"frames": frames, "runs": repeats, "seconds_median": seconds, "seconds_min": float(min(r[1] for r in runs[mode])),
                            "seconds_max": float(max(r[1] for r in runs[mode])), "frames_per_s": frames / seconds,
                            "numpy_compute_errors_seconds_median": float(np.median([r[2] for r in runs[mode]])),
                            "median_timed_forward_ms": float(np.median([r[3] for r in runs[mode]]))}
        result["device_over_host_frames_per_s"] = result["device_evaluate"]["frames_per_s"] / result["host_evaluate"]["frames_per_s"]
        result["index_lines"] = len(lines)
    return result


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--launches", type=int, default=200)
    parser.add_argument("--repeats", type=int, default=30)
    parser.add_argument("--scene-repeats", type=int, default=7)
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    parser.add_argument("--no-scene", action="store_true")
    args = parser.parse_args(argv)
    device = torch.device("cuda:0")
    os.makedirs(args.out, exist_ok=True)
    result = {"tool": "tools/evaluate_bench.py", "device": torch.cuda.get_device_name(0), "frame": f"{HEIGHT}x{WIDTH}",
              "kernel": {"N1": kernel_time(1, 1, args.launches, args.repeats, device),
                         "N64_from_hbm": kernel_time(64, 8, args.launches, args.repeats, device),
                         "N64_cache_resident": kernel_time(64, 1, args.launches, args.repeats, device)}}
    if not args.no_scene:
        result["predict_offline_24_frame_scene_device_preprocess"] = scene_throughput(device, args.scene_repeats)
    with open(os.path.join(args.out, "evaluate_bench.json"), "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()

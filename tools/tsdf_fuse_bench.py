"""Device time of batched TSDF fusion (csrc/tsdf_fuse.hip) against the per-frame kernel it reproduces, on the ``fused_scene_256`` volume of
tools/tsdf_raycast_bench.py (256^3 voxels of 1 cm) with 256x320 frames.

kernel   N sequential ``dvmvs_tsdf_integrate`` launches against ONE ``dvmvs_tsdf_integrate_frames`` call on the same device-resident frames,
         N = 1, 8, 32, both through the C ABI directly (no per-call tensor work): HIP events around each group after warm-up, medians
         over ``--reps`` groups, with both tile counters -- (tile, frame) pairs kept and tiles that loaded the volume -- next to the number
         of tiles.  The batch is checked to leave the same bits as the sequence.  The product library carries one tile shape; to compare
         shapes, build the tools-only library (``make -C deep-video-mvs_amd/csrc tuning``) and run this tool with ``DVMVS_HIP_LIB`` set
         to ``deep-video-mvs_amd/lib/libdvmvs_hip_tuning.so``: it then measures every shape that library lists.
runner   ``predict_offline`` frames per second over a synthetic 24-frame scene with ``device_preprocess=True, device_evaluate=True``, with
         and without ``fuse=`` (a LiveFusion of 2.5 cm voxels over the scene's frusta, batch 8): wall clock around the call, medians.
Prints one JSON line; ``--out PATH`` also writes it there.

    python tools/tsdf_fuse_bench.py [--reps 20] [--scene-repeats 5] [--out profiles/tsdf_fuse_bench.json]
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
for path in (os.path.join(ROOT, "deep-video-mvs_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, path)

from dvmvs.hip import _capi, ops  # noqa: E402
from dvmvs.tsdf import LiveFusion, TSDFFusion, fold_color  # noqa: E402
from tsdf_raycast_bench import H, K, W, fused_scene, views  # noqa: E402


def frames(n, dev):
    """n wavy-wall frames seen from ``views(n)``: (depth [n,H,W], rgb [n,H,W,3] uint8, folded [n,H,W], K [n,3,3], poses [n,4,4]) on the device."""
    y, x = np.meshgrid(np.arange(float(H)), np.arange(float(W)), indexing="ij")
    depth = np.stack([(1.2 + 0.2 * np.sin(x / 40 + i) + 0.1 * np.cos(y / 30)).astype(np.float32) for i in range(n)])
    rgb = np.stack([np.stack([x % 256, y % 256, (x + y + 40 * i) % 256], -1).astype(np.uint8) for i in range(n)])
    folded = np.stack([fold_color(c) for c in rgb])
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    return to(depth), to(rgb), to(folded), to(np.repeat(K[None], n, axis=0)), to(views(n))


def median_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(end))
    return [round(float(np.median(times)), 4), round(float(np.min(times)), 4), round(float(np.max(times)), 4)]


def tile_shapes(lib):
    """[(environment value or None, (tx, ty, tz))]: the product's one tile, or every shape a tuning build lists."""
    try:
        listing = lib.dvmvs_tsdf_fuse_tuning_tiles
    except AttributeError:
        return [(None, tuple(ops.TSDF_FUSE_TILE))]
    listing.restype, listing.argtypes = ctypes.c_int, [ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    xyz = (ctypes.c_int * 48)()
    count = min(listing(xyz, 16), 16)
    return [(str(i), (xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2])) for i in range(count)]


def kernel_times(dev, reps):
    lib = _capi.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    base = fused_scene(dev)
    origin, voxel, trunc = [float(o) for o in base._vol_origin], base._voxel_size, base._trunc_margin
    X, Y, Z = (int(d) for d in base._tsdf.shape)

    def clone():
        return [t.clone() for t in (base._tsdf, base._weight, base._color)]

    def dense(vol, n, data):
        depth, _, folded, Ks, Ps = data
        for i in range(n):
            _capi.check(lib.dvmvs_tsdf_integrate(vol[0].data_ptr(), vol[1].data_ptr(), vol[2].data_ptr(), X, Y, Z, *origin, voxel,
                                                 Ks[i].data_ptr(), Ps[i].data_ptr(), folded[i].data_ptr(), depth[i].data_ptr(), H, W, trunc,
                                                 1.0, stream), "dvmvs_tsdf_integrate")

    def batch(vol, n, data, workspace, stats=None):
        depth, rgb, _, Ks, Ps = data
        _capi.check(lib.dvmvs_tsdf_integrate_frames(vol[0].data_ptr(), vol[1].data_ptr(), vol[2].data_ptr(), X, Y, Z, *origin, voxel,
                                                    Ks.data_ptr(), Ps.data_ptr(), rgb.data_ptr(), None, depth.data_ptr(), n, H, W, trunc,
                                                    _capi.float_array([1.0] * n), float("inf"), workspace.data_ptr(),
                                                    None if stats is None else stats.data_ptr(), stream), "dvmvs_tsdf_integrate_frames")

    result = {"dims": [X, Y, Z], "image": [H, W], "voxels": X * Y * Z, "cases": [],
              "timing": "HIP events around N dense launches / one batched call, C ABI called directly: [median, min, max] ms"}
    for n in (1, 8, 32):
        data = frames(n, dev)
        workspace = ops.tsdf_integrate_frames_workspace(dev, n)
        row = {"n_frames": n}
        vol = clone()
        row["dense_sequence_ms"] = median_ms(lambda: dense(vol, n, data), reps)
        want = clone()
        dense(want, n, data)
        touched = int(((want[1] != base._weight) | (want[0] != base._tsdf)).sum())
        row["voxels_updated"] = touched
        # traffic if every updated voxel is read and written once (3 floats each way) against once per frame that touches it
        row["batch_volume_bytes_if_exact"] = touched * 24
        row["tiles"] = []
        for choice, tile in tile_shapes(lib):
            if choice is not None:
                os.environ["DVMVS_TSDF_FUSE_TILE"] = choice
            got, stats = clone(), torch.zeros(2, dtype=torch.int64, device=dev)
            batch(got, n, data, workspace, stats)
            equal = all(torch.equal(a, b) for a, b in zip(got, want))
            vol = clone()
            entry = {"tile": list(tile), "n_tiles": ops.tsdf_fuse_tile_count((X, Y, Z), tile), "pairs_kept": int(stats[0]),
                     "tiles_loaded": int(stats[1]), "equals_sequence_bitwise": equal,
                     "batch_ms": median_ms(lambda: batch(vol, n, data, workspace), reps)}
            entry["loaded_volume_bytes"] = entry["tiles_loaded"] * tile[0] * tile[1] * tile[2] * 12
            entry["dense_over_batch"] = round(row["dense_sequence_ms"][0] / entry["batch_ms"][0], 3)
            row["tiles"].append(entry)
        os.environ.pop("DVMVS_TSDF_FUSE_TILE", None)
        result["cases"].append(row)
    return result


def scene_throughput(dev, repeats):
    import synthetic as syn
    from preprocess_bench import _write_scene
    from dvmvs.config import Config
    from dvmvs.engine import DepthEngine
    from dvmvs.fusionnet.model import CostVolumeDecoder, CostVolumeEncoder, FeatureExtractor, FeatureShrinker, LSTMFusion
    from dvmvs.keyframe_buffer import simulate_keyframe_index, write_keyframe_index
    from dvmvs.runner import Scene, _preprocessor, predict_offline
    result = {}
    with tempfile.TemporaryDirectory() as tmp:
        folder = os.path.join(tmp, "scene")
        _write_scene(folder, 24)
        scene = Scene(folder)
        lines = simulate_keyframe_index(scene.poses, scene.image_names, Config.test_n_measurement_frames)
        index = os.path.join(tmp, "index")
        write_keyframe_index(index, lines)
        engine = DepthEngine(*syn.build_e2e_modules((FeatureExtractor, FeatureShrinker, CostVolumeEncoder, LSTMFusion, CostVolumeDecoder)),
                             device=dev)
        scaled_K = _preprocessor(scene, scene.image(0)).get_updated_intrinsics()
        bounds = TSDFFusion.frustum_bounds(list(scene.poses), scaled_K, Config.test_image_height, Config.test_image_width, 5.0) * 1.05

        def run(with_fuse):
            fuse = LiveFusion(bounds, voxel_size=0.025, max_depth=5.0, batch=8, device=dev) if with_fuse else None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            preds, _, _ = predict_offline(engine, folder, index, evaluate=True, device_preprocess=True, device_evaluate=True, fuse=fuse)
            if fuse is not None:
                fuse.flush()
            torch.cuda.synchronize()
            seconds = time.perf_counter() - t0
            dims = [int(d) for d in fuse.volume.vol_dim] if fuse is not None else None
            return len(preds), seconds, dims

        for mode in (False, True):
            run(mode)
        runs = {False: [], True: []}
        for _ in range(repeats):
            for mode in (False, True):
                runs[mode].append(run(mode))
        for mode, name in ((False, "without_fuse"), (True, "with_fuse")):
            n = runs[mode][0][0]
            seconds = float(np.median([r[1] for r in runs[mode]]))
            result[name] = {"frames": n, "runs": repeats, "seconds_median": round(seconds, 5),
                            "seconds_min": round(float(min(r[1] for r in runs[mode])), 5),
                            "seconds_max": round(float(max(r[1] for r in runs[mode])), 5), "frames_per_s": round(n / seconds, 1)}
        result["live_volume_dims"] = runs[True][0][2]
        result["live_fusion"] = {"voxel_size": 0.025, "max_depth": 5.0, "batch": 8}
        result["with_over_without_frames_per_s"] = round(result["with_fuse"]["frames_per_s"] / result["without_fuse"]["frames_per_s"], 4)
    return result


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scene-repeats", type=int, default=5)
    ap.add_argument("--no-scene", action="store_true", help="kernel times only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "scene": "fused_scene_256", "kernel": kernel_times(dev, args.reps)}
    if not args.no_scene:
        out["predict_offline_24_frame_scene"] = scene_throughput(dev, args.scene_repeats)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

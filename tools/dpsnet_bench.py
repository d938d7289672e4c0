"""Device time of the DPSNet baseline (dvmvs.baselines.dpsnet) and of its two kernels (csrc/dps_volume.hip, csrc/dps_regress.hip).

* frame: one frame at 320x240, M = 1 and 2 measurement frames, seeded weights, HIP events around --reps calls after warm-up,
  (i) on the fused route and (ii) on the plain-torch route with the same tensors on the device (the reference's formulation: the
  baseline), the two alternating in one timed loop.
* kernels: dvmvs::dps_volume (C = 32, 64 planes, 60x80) against the plain route's per-plane loop and against a device copy of the same
  78.6 MB in the same run; dvmvs::dps_regress (64 planes, 60x80 -> 240x320) against the plain route's interpolate / softmax / sum.
* --trace-frames N: nothing is timed; N frames per route run between dvmvs_trace_marker launches, for
      rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/dpsnet_bench.py --trace-frames 3
  whose CSVs ``--summarise DIR`` turns into launches per frame and the two kernels' times.
Prints one JSON line; ``--out PATH`` also writes it there.

    python tools/dpsnet_bench.py [--reps 10] [--out profiles/dpsnet_bench.json]
"""
import argparse
import csv
import glob
import json
import os
import sys

import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
for p in (os.path.join(ROOT, "deep-video-mvs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import dpsnet_fixtures as fx  # noqa: E402
import synthetic as syn  # noqa: E402
from dvmvs.baselines import runner  # noqa: E402
from dvmvs.hip import _capi, ops  # noqa: E402

HBM_ACHIEVABLE = 6.3e12
H, W = 240, 320


def time_ms(fns, reps, warmup=2):
    """Mean device time per call of each function, the functions alternating inside one loop."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    totals = [0.0] * len(fns)
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns]
    for _ in range(reps):
        for (start, end), fn in zip(events, fns):
            start.record()
            fn()
            end.record()
        torch.cuda.synchronize()
        for i, (start, end) in enumerate(events):
            totals[i] += start.elapsed_time(end)
    return [t / reps for t in totals]


def frame_inputs(dev, M):
    r, ms = syn.keyframe_index_lines(2)[0]
    K, Kinv = fx.intrinsics(W, H)
    return (fx.e2e_image(r, H, W).to(dev), [fx.e2e_image(m, H, W).to(dev) for m in ms[:M]], [fx.relative_pose(r, m).to(dev) for m in ms[:M]],
            K.to(dev), Kinv.to(dev))


def run_route(net, route, inputs):
    net.route = route
    with torch.no_grad():
        return net(*inputs)


def frame_rows(dev, reps):
    net = runner.build_dpsnet(None, dev)
    rows = []
    for M in (1, 2):
        inputs = frame_inputs(dev, M)
        fused, plain = time_ms([lambda: run_route(net, "fused", inputs), lambda: run_route(net, "plain", inputs)], reps)
        rows.append({"M": M, "fused_ms": round(fused, 3), "plain_torch_ms": round(plain, 3), "speedup": round(plain / fused, 2)})
    return rows


def kernel_rows(dev, reps):
    net = runner.build_dpsnet(None, dev)
    ref, meas = (t.to(dev) for t in fx.feature_maps(1, 32, 60, 80, seed=300))
    K4, Kinv4 = (t.to(dev) for t in fx.quarter(*fx.intrinsics(W, H)))
    pose = fx.relative_pose(9, 6).to(dev)
    volume = ops.dps_volume(ref, meas, pose, K4, Kinv4, fx.NLABEL, fx.MINDEPTH)
    copy = torch.empty_like(volume)
    costs = fx.regress_costs("random", fx.NLABEL, 60, 80, seed=500).to(dev)
    with torch.no_grad():
        t_volume, t_loop, t_copy, t_regress, t_chain = time_ms([
            lambda: ops.dps_volume(ref, meas, pose, K4, Kinv4, fx.NLABEL, fx.MINDEPTH),
            lambda: net.plane_volume(ref, meas, pose, K4, Kinv4),
            lambda: copy.copy_(volume),
            lambda: ops.dps_regress(costs, H, W, fx.MINDEPTH),
            lambda: net.regress(costs, H, W)], reps)
    nbytes = volume.numel() * 4
    return {"dps_volume_us": round(t_volume * 1e3, 1), "plain_volume_loop_us": round(t_loop * 1e3, 1),
            "device_copy_same_bytes_us": round(t_copy * 1e3, 1), "volume_bytes": nbytes,
            "write_floor_us": round(nbytes / HBM_ACHIEVABLE * 1e6, 1),
            "dps_regress_us": round(t_regress * 1e3, 1), "plain_regress_chain_us": round(t_chain * 1e3, 1)}


def trace(dev, frames):
    net = runner.build_dpsnet(None, dev)
    inputs = frame_inputs(dev, 2)
    lib, stream = _capi.lib(), torch.cuda.current_stream(dev).cuda_stream
    for route in ("fused", "plain"):
        run_route(net, route, inputs)                       # warm-up: MIOpen's choices, code objects
    torch.cuda.synchronize()
    for route in ("fused", "plain"):
        lib.dvmvs_trace_marker(stream)
        for _ in range(frames):
            run_route(net, route, inputs)
        torch.cuda.synchronize()
    lib.dvmvs_trace_marker(stream)
    torch.cuda.synchronize()


def summarise(folder, frames):
    """Launches per frame of the two routes (between the trace markers), the mean time of the two kernels and the largest kernels of a
    frame, from rocprofv3's kernel-trace CSV."""
    files = glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {folder}")
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        r["ns"] = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    marks = [i for i, r in enumerate(rows) if "trace_marker_kernel" in r["Kernel_Name"]]
    out = {}
    for route, (a, b) in zip(("fused", "plain"), zip(marks, marks[1:])):
        seg = rows[a + 1:b]
        out[route] = {"launches_per_frame": len(seg) / frames, "kernel_time_ms_per_frame": round(sum(r["ns"] for r in seg) / frames / 1e6, 3)}
        for name in ("dps_volume_kernel", "dps_regress_kernel"):
            t = [r["ns"] for r in seg if name in r["Kernel_Name"]]
            if t:
                out[route][name + "_us"] = round(sum(t) / len(t) / 1e3, 1)
                out[route][name + "_launches_per_frame"] = len(t) / frames
        top = {}
        for r in seg:
            top[r["Kernel_Name"][:80]] = top.get(r["Kernel_Name"][:80], 0) + r["ns"]
        out[route]["top_kernels_ms_per_frame"] = {k: round(v / frames / 1e6, 3) for k, v in sorted(top.items(), key=lambda kv: -kv[1])[:6]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--trace-frames", type=int, default=0)
    ap.add_argument("--summarise", default=None, help="folder of a rocprofv3 --kernel-trace run of --trace-frames")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.summarise:
        result = summarise(args.summarise, args.trace_frames or 3)
    else:
        if not torch.cuda.is_available():
            raise SystemExit("dpsnet_bench needs an MI355X")
        dev = torch.device("cuda:0")
        if args.trace_frames:
            trace(dev, args.trace_frames)
            return
        result = {"device": torch.cuda.get_device_name(dev), "shape": "1x3x240x320, 64 planes, mindepth 0.5, seeded weights",
                  "frame": frame_rows(dev, args.reps), "kernels": kernel_rows(dev, args.reps)}
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

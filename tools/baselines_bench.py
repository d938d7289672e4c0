"""Device time of the MVDepthNet / GP-MVS baselines (dvmvs.baselines) and of their RGB SAD sweep (csrc/sweep_rgb.hip).

* sweep: dvmvs::rgb_sweep against the generic SAD kernel (dvmvs_cost_volume_fwd variant 1, the only SAD path before it) at
  320x256, 64 planes, M = 1, 2, 3, HIP events around --reps calls after warm-up; the floor is the 64 x 320 x 256 x 4 B = 21 MB write
  at 6.3 TB/s (the achievable HBM rate; 8 TB/s peak).
* frames: frames/s of both baselines on a synthetic sequence (seeded weights, synthetic.e2e_image inputs, sample-scene poses,
  two measurement frames), and the per-frame split between sweep, encoder, filter and decoder, each bracketed by HIP events.
Prints one JSON line; ``--out PATH`` also writes it there.

    python tools/baselines_bench.py [--reps 50] [--frames 40] [--out profiles/baselines_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
for p in (os.path.join(ROOT, "deep-video-mvs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import synthetic as syn  # noqa: E402
from dvmvs.baselines import runner  # noqa: E402
from dvmvs.hip import ops  # noqa: E402
from dvmvs.pose_algebra import sweep_matrices_host  # noqa: E402

HBM_ACHIEVABLE = 6.3e12


def time_us(fn, reps):
    for _ in range(3):
        fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1000.0 / reps


def sweep_rows(dev, reps):
    rows = []
    lines = syn.keyframe_index_lines(3)
    r, ms = lines[1]
    K = syn.full_K()
    for M in (1, 2, 3):
        Hm, kt = sweep_matrices_host(syn.pose(r), [syn.pose(m) for m in ms[:M]], K)
        Hm, kt = Hm.to(dev), kt.to(dev)
        ref = syn.e2e_image(r).to(dev)
        meas = [syn.e2e_image(m).to(dev) for m in ms[:M]]
        fused = torch.empty((1, 67, 256, 320), device=dev)
        new = time_us(lambda: ops.rgb_sweep(fused, ref, meas, Hm, kt, 0.5, 50.0, 64, 3, True), reps)
        plain = torch.empty((1, 64, 256, 320), device=dev)
        new_plain = time_us(lambda: ops.rgb_sweep(plain, ref, meas, Hm, kt, 0.5, 50.0, 64, 0, False), reps)
        generic = time_us(lambda: ops.cost_volume(ref, meas, Hm, kt, 0.5, 50.0, 64, False, 1), reps)
        same = torch.equal(fused[:, 3:], ops.cost_volume(ref, meas, Hm, kt, 0.5, 50.0, 64, False, 1))
        floor_us = 64 * 256 * 320 * 4 / HBM_ACHIEVABLE * 1e6
        rows.append({"M": M, "rgb_sweep_fused_us": round(new, 2), "rgb_sweep_plain_us": round(new_plain, 2), "generic_sad_us": round(generic, 2),
                     "speedup_plain_vs_generic": round(generic / new_plain, 2), "write_floor_us": round(floor_us, 2),
                     "fraction_of_write_floor_plain": round(floor_us / new_plain, 3), "bit_identical_to_generic": bool(same)})
    return rows


def frame_rows(dev, n_frames):
    poses = syn.sample_poses()
    lines = syn.keyframe_index_lines(2)[:n_frames]
    K = syn.full_K()
    images = {i: syn.e2e_image(i).to(dev) for line in lines for i in (line[0], *line[1])}
    pose = {i: torch.from_numpy(poses[i]).float().unsqueeze(0) for i in images}     # host tensors, parsed once
    out = {}
    for method in ("mvdepthnet", "gpmvs"):
        if method == "mvdepthnet":
            enc, dec = runner.build_mvdepthnet(None, dev)
            frame = runner.BaselineFrame(enc, dec, dev)
        else:
            enc, dec, gpl = runner.build_gpmvs(None, dev)
            frame = runner.BaselineFrame(enc, dec, dev, gp=runner.GPFilter.from_gplayer(gpl))

        def run(r, ms, dt):
            return frame(images[r], [images[m] for m in ms], pose[r], [pose[m] for m in ms], K, dt=dt)

        with torch.no_grad():
            for r, ms in lines[:3]:
                run(r, ms, 0.15)
            torch.cuda.synchronize()
            # frames/s: the whole loop, one synchronise at the end
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            prev = None
            for r, ms in lines:
                dt = runner.pose_distance(poses[r], poses[prev if prev is not None else ms[-1]])[0]
                run(r, ms, dt)
                prev = r
            end.record()
            end.synchronize()
            total_ms = start.elapsed_time(end)
            # per-stage split: events between the stages of the same frame order
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
            split = {"sweep": 0.0, "encoder": 0.0, "filter": 0.0, "decoder": 0.0}
            for r, ms in lines:
                ev[0].record()
                fused = frame.sweep(images[r], [images[m] for m in ms], pose[r], [pose[m] for m in ms], K)
                ev[1].record()
                c5, c4, c3, c2, c1 = enc.forward_fused(fused)
                ev[2].record()
                if frame.gp is not None:
                    A, k, reset = frame.gp.step(0.15)
                    c5 = ops.gp_filter_step(frame.state, c5.reshape(-1), A, k, reset).view_as(c5)
                ev[3].record()
                1.0 / torch.clamp(dec(c5, c4, c3, c2, c1)[0], 0.02, 2.0)
                ev[4].record()
                ev[4].synchronize()
                for i, key in enumerate(split):
                    split[key] += ev[i].elapsed_time(ev[i + 1]) / len(lines)
        frame_ms = total_ms / len(lines)
        out[method] = {"frames": len(lines), "ms_per_frame": round(frame_ms, 3), "frames_per_s": round(1000.0 / frame_ms, 1),
                       "split_ms": {k: round(v, 3) for k, v in split.items()},
                       "split_share": {k: round(v / sum(split.values()), 3) for k, v in split.items()}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("baselines_bench needs an MI355X")
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(dev), "shape": "1x3x256x320, 64 planes, 0.5-50 m",
              "sweep": sweep_rows(dev, args.reps), "baselines": frame_rows(dev, args.frames)}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

"""Generates tests/golden/engine_sizes_<W>x<H>.npz (results) and engine_sizes_<W>x<H>_state.npz (installed state): the frames of tests/engine_size_cases.py through the CPU oracle pipeline
(oracle/fusionnet_cpu.CpuDepthPipeline on this package's modules) in float32 and in float64, per frame size.

    python tests/golden/make_engine_size_goldens.py                 # all sizes
    python tests/golden/make_engine_size_goldens.py 96x64 160x128   # some

Runs on the CPU; nothing but this repository is read.  Per size and frame the files hold
* ``f<n>_state_{h_q,c_q,depth_q}``, ``f<n>_state_pose`` (n >= 1): the state installed before the frame -- the float32 pipeline's state after frame
  n - 1, rounded as engine_size_cases.pack_state says -- which BOTH pipelines (and the engine under test) start the frame from (teacher forcing);
* the float64 results rounded to float32: ``f<n>_{depth,depth_border,depth_blocks}64`` (engine_size_cases.depth_values: the drawn pixels or the
  whole map, the two-pixel border, the 8x8 block means), ``f<n>_depth64_sum``, ``f<n>_depth_estimation`` (whole), and
  ``f<n>_{h,c,bottom,cost_volume,feat_half}64_samples`` / ``_sum`` / ``_abs_sum`` (the sums over the whole tensor);
* ``f<n>_<stage>_yardstick``: the float32 pipeline's own distance from the float64 one on exactly those stored values -- what "equal up to fp32
  round-off" means at this size; the tests allow the engine engine_size_cases.SLACK times the largest over the size's frames;
* ``f<n>_estimate_flips``: pixels of the low-resolution depth estimate on which the two pipelines differ (asserted 0 here: the tests demand 0).
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.dirname(HERE), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "deep-video-mvs_amd")):
    sys.path.insert(0, p)

import engine_size_cases as cases  # noqa: E402
import synthetic as syn  # noqa: E402

torch.set_num_threads(min(16, os.cpu_count() or 1))


def modules():
    from dvmvs.fusionnet.model import CostVolumeDecoder, CostVolumeEncoder, FeatureExtractor, FeatureShrinker, LSTMFusion
    return syn.build_e2e_modules((FeatureExtractor, FeatureShrinker, CostVolumeEncoder, LSTMFusion, CostVolumeDecoder))


def size_arrays(W, H, state_from=None):
    """(the fixture's arrays of one size, {name: the float64 values before their rounding to float32}).  ``state_from``: a fixture whose installed
    state is used instead of this run's own (tests/test_engine_sizes_host.py re-derives a fixture's results on another CPU, whose float32 pipeline
    rounds a few state values the other way)."""
    from fusionnet_cpu import CpuDepthPipeline
    mods = modules()
    pipe32 = CpuDepthPipeline(*mods)
    pipe64 = CpuDepthPipeline(*[copy.deepcopy(m).double() for m in mods])
    K = cases.full_K(W, H)
    arrays, exact = {}, {}
    for n, (r, ms) in enumerate(cases.frames(W, H)):
        if n > 0:      # teacher forcing: both pipelines continue from the float32 pipeline's state, rounded to what the fixture stores
            packed = cases.pack_state(pipe32.lstm_state[0], pipe32.lstm_state[1], pipe32.previous_depth)
            if state_from is not None:
                packed = {k: state_from[f"f{n}_state_{k}"] for k in packed}
            arrays.update({f"f{n}_state_{k}": v for k, v in packed.items()})
            arrays[f"f{n}_state_pose"] = pipe32.previous_pose.numpy()
            h, c, depth = cases.unpack_state(arrays, f"f{n}_state")
            for pipe, cast in ((pipe32, torch.Tensor.float), (pipe64, torch.Tensor.double)):
                pipe.lstm_state, pipe.previous_depth = (cast(h), cast(c)), cast(depth).view(1, 1, H, W)
                pipe.previous_pose = cast(torch.from_numpy(arrays[f"f{n}_state_pose"]))
        rec32, rec64 = {}, {}
        args = (cases.image(r, W, H), syn.pose(r), [cases.image(i, W, H) for i in ms], [syn.pose(i) for i in ms], K)
        pipe32.step(*args, record=lambda **kw: rec32.update(kw))
        pipe64.step(args[0].double(), args[1].double(), [t.double() for t in args[2]], [t.double() for t in args[3]], K.double(),
                    record=lambda **kw: rec64.update(kw))
        d32, d64 = (cases.depth_values(rec["depth"], W, H) for rec in (rec32, rec64))
        for stage in cases.DEPTH_STAGES:
            arrays[f"f{n}_{stage}64"], exact[f"f{n}_{stage}64"] = d64[stage].astype(np.float32), d64[stage]
            arrays[f"f{n}_{stage}_yardstick"] = cases.depth_distance(d32[stage], d64[stage])
        arrays[f"f{n}_depth64_sum"] = d64["sum"]
        arrays[f"f{n}_depth_estimation"] = rec64["depth_estimation"].float().numpy()
        flips = cases.flipped_pixels(rec32["depth_estimation"].numpy(), rec64["depth_estimation"].numpy())
        arrays[f"f{n}_estimate_flips"] = flips
        assert flips == 0, (W, H, n, flips)
        for stage in cases.SAMPLED:
            s32, s64 = cases.samples(rec32[stage]), cases.samples(rec64[stage])
            arrays[f"f{n}_{stage}64_samples"], exact[f"f{n}_{stage}64_samples"] = s64.astype(np.float32), s64
            arrays[f"f{n}_{stage}64_sum"] = float(rec64[stage].sum())
            arrays[f"f{n}_{stage}64_abs_sum"] = float(rec64[stage].abs().sum())
            arrays[f"f{n}_{stage}_yardstick"] = cases.distance(s32, s64)
        print(f"{W}x{H} frame {n}: float32 vs float64 " + ", ".join(f"{s} {float(arrays[f'f{n}_{s}_yardstick']):.2e}" for s in cases.STAGES) +
              f"; estimate flips {flips}; depth {d64['depth'].min():.3f} .. {d64['depth'].max():.3f}", flush=True)
    return arrays, exact


def main(argv):
    wanted = [tuple(int(v) for v in a.split("x")) for a in argv] or cases.SIZES
    for W, H in wanted:
        arrays, _ = size_arrays(W, H)
        for path, keep in ((cases.fixture_path(W, H, HERE), lambda name: not cases.is_state(name)), (cases.state_path(W, H, HERE), cases.is_state)):
            np.savez_compressed(path, **{name: a for name, a in arrays.items() if keep(name)})
            size = os.path.getsize(path)
            print(f"wrote {os.path.basename(path)}: {size / 1024:.0f} KiB", flush=True)
            assert size < 1024 * 1024, "a committed file stays under 1 MiB"


if __name__ == "__main__":
    main(sys.argv[1:])

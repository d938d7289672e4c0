"""Do eight host loops fit the machine?  

At N = 8 every rank runs the engine's host path once per frame -- the reference's fp32 pose algebra (~40 small torch operations), the sweep's
launch plan, the parameter block build, and a graph launch -- and the frame is co-bound by it (0.74 ms of host time against 0.78 ms of device
time per frame at N = 1).  The GPUs do not share anything; the host cores do.  This test runs the HOST half of ``DepthEngine.step`` (the very
function the engine calls, ``ParameterBlock.evaluate``, on the keyframe poses of the sample scene, + the mirror copy + a stubbed launch that
sleeps without the interpreter lock, as hipGraphLaunch does) in 1 and in 8 processes at once, one torch thread each as ``bench.py`` configures
them per rank, and reports the per-step host time.  No device involved: the scaling of the host part is what is measured.
Reference loop: /root/reference/dvmvs/fusionnet/run-testing.py:151-204 (its pose algebra: utils.py:51-56, :121, convlstm.py:30)."""
import json
import multiprocessing as mp
import os
import sys
import time

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS, LAUNCH_STUB_SECONDS, REPEATS = 600, 0.0004, 3


def _host_loop(rank, queue, barrier, core):
    if core is not None:
        os.sched_setaffinity(0, {core})      # a core of its own, as "a machine with at least eight usable cores" gives every rank
    sys.path[:0] = [os.path.join(HERE, "..", "deep-video-mvs_amd"), HERE]
    import torch
    torch.set_num_threads(1)
    import synthetic as syn
    from dvmvs.parameter_block import ParameterBlock
    block = ParameterBlock(sequences=1, height=256, width=320, n_depth_levels=64, min_depth=0.25, max_depth=20.0, pose_algebra="reference",
                           sweep_work_list=True, sweep_mfma=True, is_fusionnet=True)      # (fusionnet: the two relative poses as well)
    mirror, staging = block.mirror, torch.zeros(block.total)
    poses = torch.from_numpy(syn.sample_poses()).float()
    lines = syn.keyframe_index_lines(2)
    full_K = syn.full_K()
    previous = poses[lines[0][0]:lines[0][0] + 1]
    no_previous = torch.zeros(1, dtype=torch.bool)
    for k in range(5):      # warm-up: library load, LAPACK, allocator
        r, ms = lines[k]
        block.evaluate(mirror, 2, poses[r:r + 1], [poses[m:m + 1] for m in ms], full_K, previous, no_previous, 0, True, None)
    barrier.wait()
    t0 = time.perf_counter()
    busy = 0.0
    for k in range(STEPS):
        r, ms = lines[(5 + k + 31 * rank) % len(lines)]
        t1 = time.perf_counter()
        committed, variant, _ = block.evaluate(mirror, 2, poses[r:r + 1], [poses[m:m + 1] for m in ms], full_K, previous, no_previous, k & 1, True, None)
        staging.copy_(mirror)
        busy += time.perf_counter() - t1
        time.sleep(LAUNCH_STUB_SECONDS)      # the graph launch: the interpreter lock is released, the core is not needed
        previous = committed
        assert variant == 6
    queue.put((rank, (time.perf_counter() - t0) / STEPS * 1e3, busy / STEPS * 1e3))


def _run(n):
    ctx = mp.get_context("spawn")
    queue, barrier = ctx.Queue(), ctx.Barrier(n)
    # one rank per usable core where there are enough of them (the scheduler otherwise stacks two ranks on one core now and then, and the
    # test measures where they were put, not the host path)
    cores = sorted(os.sched_getaffinity(0)) if hasattr(os, "sched_setaffinity") else []
    pin = [cores[rank] for rank in range(n)] if len(cores) >= n else [None] * n
    procs = [ctx.Process(target=_host_loop, args=(rank, queue, barrier, pin[rank])) for rank in range(n)]
    for p in procs:
        p.start()
    results = [queue.get(timeout=300) for _ in range(n)]
    for p in procs:
        p.join(timeout=60)
    return sorted(results)


def test_eight_host_loops_cost_per_rank_what_one_costs():
    # REPEATS interleaved rounds of one rank alone and eight at once, so that a slow or a quiet spell of a shared machine falls on both sides;
    # of each, the median round counts (one round of either alone varies by a third from run to run on a virtual machine)
    rounds_1, rounds_8 = [], []
    for _ in range(REPEATS):
        rounds_1.append(_run(1))
        rounds_8.append(_run(8))
    one = sorted(rounds_1, key=lambda r: r[0][2])[REPEATS // 2]
    eight = sorted(rounds_8, key=lambda r: max(x[2] for x in r))[REPEATS // 2]
    step_1, busy_1 = one[0][1], one[0][2]
    step_8, busy_8 = max(r[1] for r in eight), max(r[2] for r in eight)
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    report = {"host_cores_visible": cores, "steps": STEPS, "rounds": REPEATS, "launch_stub_ms": LAUNCH_STUB_SECONDS * 1e3,
              "one_rank": {"ms_per_step": round(step_1, 4), "host_work_ms_per_step": round(busy_1, 4)},
              "eight_ranks_worst": {"ms_per_step": round(step_8, 4), "host_work_ms_per_step": round(busy_8, 4)},
              "eight_ranks_all": [round(r[2], 4) for r in eight]}
    print("\nhost path, 1 vs 8 concurrent ranks: " + json.dumps(report))
    out = os.environ.get("DVMVS_HOST_SCALING_REPORT")
    if out:
        with open(out, "w") as f:
            json.dump(report, f, indent=1)
    # every rank's host work per frame (pose algebra + plan + block build, one thread) must stay well inside a 0.8 ms frame with eight of them running,
    # and must not degrade by more than half against one rank alone on a machine with at least eight usable cores
    assert busy_8 < 1.0, report
    if cores >= 8:
        assert busy_8 < 1.5 * busy_1 + 0.05, report

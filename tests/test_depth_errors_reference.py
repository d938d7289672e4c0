"""CPU: pins the term-exact float64 reference of tests/depth_errors_reference.py (what tests/test_depth_errors_gpu.py measures the kernel
against) to the product's host function and to the reference's recorded metrics, and covers the host-side plumbing of device evaluation
-- save_results(errors=...), the deferred InferenceTimer, and the scene runner's bookkeeping with a stub engine and the op replaced by
the reference."""
import os

import numpy as np
import pytest
import torch

import depth_errors_reference as ref
import synthetic as syn

# |compute_errors - reference| / |reference| allowed per case.  The two share every float32 term; compute_errors adds them pairwise in
# float32 (error of a few roundings, each 2^-24 relative), the reference adds them in float64: 4 * 2^-23 (measured: at most 1.8 * 2^-23,
# on the 91-pixel frame).  A one-pixel frame has nothing to add up -- the mean of one term is the term -- and differs only by the
# double rounding of rmse (sqrt in float64, then float32, against sqrt in float32): one spacing.
HOST_BOUND = {case: 4 * ref.U for case in ref.CASES}
HOST_BOUND["one_pixel"] = ref.U


@pytest.mark.parametrize("case", sorted(ref.CASES))
def test_reference_against_compute_errors(case):
    worst = 0.0
    for N in ref.BATCHES:
        gts, preds = ref.batch(case, N)
        for max_depth in ref.MAX_DEPTHS:
            for gt, pred in zip(gts, preds):
                metrics, counts = ref.reference(gt, pred, max_depth)
                host = ref.host_errors(gt, pred, max_depth)
                keep = (gt >= 0.5) & (gt <= max_depth)
                assert counts[0] == int(keep.sum())
                if counts[0] == 0:
                    assert np.isnan(metrics).all() and np.isnan(host).all() and not counts.any()
                    continue
                # the counts compute_errors' ratios imply (count / float32(n), n < 2^24: count = round(ratio * n) exactly)
                assert [int(round(float(host[5 + k]) * counts[0])) for k in range(3)] == list(counts[1:])
                assert metrics.dtype == np.float32 and np.isfinite(metrics).all() and np.isfinite(host).all()
                exact = metrics.astype(np.float64)
                assert np.array_equal(host[exact == 0], exact[exact == 0])          # (a ratio without inliers)
                rel = np.abs(host - exact)[exact != 0] / np.abs(exact[exact != 0])
                worst = max(worst, float(rel.max()))
                assert np.array_equal(metrics[5:], (counts[1:].astype(np.float32) / np.float32(counts[0])))
    print(f"{case}: max |compute_errors - reference| / |reference| = {worst / ref.U:.2f} * 2^-23 (bound {HOST_BOUND[case] / ref.U:.0f})")
    assert worst <= HOST_BOUND[case]
    assert ref.reference(*ref.frame("one_pixel"))[1][0] == 1


def test_reference_reproduces_the_recorded_metrics(golden_dir):
    """tests/golden/error_metrics.npz: the reference's compute_errors on the float64 inputs of syn.error_metric_inputs().  The reference here
    sees them rounded to float32: each of gt, pred moves by 2^-24 relative, d = gt - pred by up to 2^-24 (gt + pred), the mean of |d| by up
    to 2^-24 mean(gt + pred) / mean|d| relative (the condition number of the fixture, ~30), squares by twice that; the terms' own float32
    roundings add at most four more 2^-24.  The counts are reproduced exactly."""
    z = np.load(os.path.join(golden_dir, "error_metrics.npz"))
    gt, pred = syn.error_metric_inputs()
    for key, max_depth in (("all_pixels", np.inf), ("max_depth_2", 2.0)):
        keep = (gt >= 0.5) & (gt <= max_depth)
        condition = float(np.mean((gt + pred)[keep]) / np.mean(np.abs(gt - pred)[keep]))
        bound = (2 * condition + 4) * 2.0 ** -24
        metrics, counts = ref.reference(gt.astype(np.float32), pred.astype(np.float32), max_depth)
        rel = np.abs(metrics.astype(np.float64) - z[key]) / np.abs(z[key])
        print(f"{key}: max relative difference {rel.max():.2e} (bound {bound:.2e})")
        assert rel[:5].max() <= bound
        assert np.array_equal(metrics[5:], z[key][5:].astype(np.float32)) and counts[0] == int(keep.sum())
    assert np.isnan(z["nothing_valid"]).all() and np.isnan(ref.reference(np.zeros((4, 4), np.float32), np.ones((4, 4), np.float32))[0]).all()


def test_special_cases_on_the_host():
    """nothing_valid and all_clipped give eight NaNs; non_finite gives the recorded inf / NaN pattern in numpy and in the reference."""
    for gt, pred, max_depth in ((*ref.nothing_valid(), np.inf), (*ref.frame("ragged_multi"), ref.ALL_CLIPPED_MAX_DEPTH)):
        metrics, counts = ref.reference(gt, pred, max_depth)
        assert ref.pattern(metrics) == "n" * 8 == ref.pattern(ref.host_errors(gt, pred, max_depth)) and not counts.any()
    base_counts = ref.reference(*ref.frame("ragged_multi"))[1]
    for name, (edits, want) in ref.NON_FINITE.items():
        gt, pred = ref.non_finite(name)
        metrics, counts = ref.reference(gt, pred)
        host = ref.host_errors(gt, pred)
        assert ref.pattern(metrics) == want == ref.pattern(host), name
        ref.check_against_host(metrics, metrics, host)
        assert abs(int(counts[0]) - int(base_counts[0])) <= len(edits)
        assert [int(round(float(host[5 + k]) * counts[0])) for k in range(3)] == list(counts[1:])


def test_save_results_takes_evaluated_rows(tmp_path):
    from dvmvs.utils import save_results
    gts, preds = ref.batch("sub_wave", 3)
    rows = [np.array(ref.host_errors(g, p), dtype=np.float32) for g, p in zip(gts, preds)]
    for tag, errors in (("recomputed", None), ("given", rows)):
        (tmp_path / tag).mkdir()
        save_results(list(preds), list(gts), "system", "scene", str(tmp_path / tag), errors=errors)
    for name in ("system_errors_scene.npz", "system_predictions_scene.npz"):
        a, b = np.load(tmp_path / "recomputed" / name)["arr_0"], np.load(tmp_path / "given" / name)["arr_0"]
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b), name
    assert np.load(tmp_path / "given" / "system_errors_scene.npz")["arr_0"].shape == (3, 8)
    with pytest.raises(ValueError):
        save_results(list(preds), list(gts), "system", "scene", str(tmp_path), errors=rows[:2])


def test_deferred_timer_on_the_cpu_branch(monkeypatch):
    """Without a GPU both timers are the wall-clock stop-watch: same times, same statistics; resolve() is a no-op."""
    from dvmvs import utils
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    stats = []
    for deferred in (False, True):
        ticks = iter(np.cumsum([0.0, 0.010, 0.5, 0.013, 0.25, 0.007, 1.0, 0.021]))
        monkeypatch.setattr(utils.time, "perf_counter", lambda: float(next(ticks)))
        timer = utils.InferenceTimer(n_skip=1, deferred=deferred)
        for _ in range(4):
            timer.record_start_time()
            timer.record_end_time_and_elapsed_time()
        timer.resolve()
        assert len(timer.times) == 4 and all(t > 0 for t in timer.times)
        stats.append((list(timer.times), timer.statistics()))
    assert stats[0] == stats[1] and stats[0][1]["n"] == 3 and abs(stats[0][1]["max"] - 21.0) < 1e-6
    assert utils.InferenceTimer(deferred=True).statistics() is None


class _StubEngine:
    """Stands in for DepthEngine on the CPU.  ``static``: one output buffer that every step overwrites, as the engine's is (the default
    path's ``.cpu()`` of a CPU tensor would alias it, so that path gets a fresh tensor per step)."""
    cache_features = False

    def __init__(self, static=False):
        self.static = static
        self.device = torch.device("cpu")
        self.output = torch.zeros((1, 1, 256, 320))
        self.resets = 0

    def new_sequence(self):
        pass

    def reset(self):
        self.resets += 1

    def step(self, reference_image, reference_pose, measurement_images, measurement_poses, full_K, frame_id=None, **kwargs):
        self.output.copy_(1.6 + 0.05 * frame_id + 0.1 * reference_image.mean(1, keepdim=True))
        return self.output if self.static else self.output.clone()


def _reference_op(gt, pred, max_depth=float("inf"), out=None, counts=None):
    rows = ref.reference_batch(gt.reshape(-1, *gt.shape[-2:]).numpy(), pred.reshape(-1, *pred.shape[-2:]).numpy(), max_depth)[0]
    out.copy_(torch.from_numpy(rows))
    return out


def test_runner_bookkeeping_with_a_stub_engine(monkeypatch, tmp_path):
    """predict_offline / predict_online with device_evaluate on a CPU stub: same predictions and ground truth as the default path, one
    row per prediction that obeys the triangle rule against compute_errors, the deferred timer filled in, and an empty error_log without
    ground truth or with evaluate=False."""
    from test_runner import _write_scene
    from dvmvs.hip import ops
    from dvmvs.runner import predict_offline, predict_online
    monkeypatch.setattr(ops, "depth_errors", _reference_op)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # the stop-watch's CPU branch, wherever this runs
    scene = str(tmp_path / "scene")
    _write_scene(scene, 14)
    index = str(tmp_path / "index")
    with open(index, "w") as f:
        f.write("00009.png 00006.png 00003.png\n00010.png 00009.png 00006.png\nTRACKING LOST\n00013.png 00010.png 00009.png\n")
    runs = {"offline": lambda **kw: predict_offline(_StubEngine("device_evaluate" in kw), scene, index, evaluate=True, **kw),
            "online": lambda **kw: predict_online(_StubEngine("device_evaluate" in kw), scene, evaluate=True, **kw)}
    for what, run in runs.items():
        preds, gts, timer = run()
        rows = []
        preds_dev, gts_dev, timer_dev = run(device_evaluate=True, error_log=rows)
        assert len(preds) == len(preds_dev) == len(gts_dev) == len(rows) == len(timer_dev.times) >= 3 and len(timer.times) == len(preds)
        assert not np.array_equal(preds[0], preds[1])        # the stub's static buffer was copied out frame by frame
        for p, g, pd, gd, row in zip(preds, gts, preds_dev, gts_dev, rows):
            assert pd.shape == (256, 320) and np.array_equal(p, pd) and gd.dtype == g.dtype and np.array_equal(g, gd)
            assert row.dtype == np.float32 and row.shape == (8,)
            ref.check_against_host(row, ref.reference(g.astype(np.float32), p)[0], ref.host_errors(g, p))
        assert all(t > 0 for t in timer_dev.times)
    rows = []
    preds, gts, _ = predict_offline(_StubEngine(True), scene, index, evaluate=False, device_evaluate=True, error_log=rows)
    assert len(preds) == 3 and gts is None and rows == []
    import shutil
    shutil.rmtree(os.path.join(scene, "depth"))
    preds, gts, _ = predict_offline(_StubEngine(True), scene, index, evaluate=True, device_evaluate=True, error_log=rows)
    assert len(preds) == 3 and gts is None and rows == []


class _StubBaselineFrame:
    """Stands in for BaselineFrame on the CPU: MVDepthNet's attributes, and a depth that depends on the reference image and pose, written
    into ONE static buffer (``static``) as the networks' outputs may be."""
    gp = None

    def __init__(self, static=False):
        self.static = static
        self.device = torch.device("cpu")
        self.output = torch.zeros((1, 1, 256, 320))

    def __call__(self, reference_image, measurement_images, reference_pose, measurement_poses, K, dt=None):
        assert dt is None and len(measurement_images) == len(measurement_poses) == 2 and not torch.is_grad_enabled()
        self.output.copy_(1.6 + 0.05 * reference_pose.abs().sum() + 0.001 * reference_image.mean(1, keepdim=True))
        return self.output if self.static else self.output.clone()


def test_baseline_loop_bookkeeping_with_a_stub_frame(monkeypatch, tmp_path):
    """The baselines' loop with device_evaluate on a CPU stub: same predictions and ground truth (array and dtype) as the default path, one
    row per prediction that obeys the triangle rule against compute_errors, one positive time per prediction, and an empty error_log
    without ground truth or with evaluate=False."""
    import shutil
    from test_runner import _write_scene
    from dvmvs.baselines.runner import _predict_baseline
    from dvmvs.hip import ops
    monkeypatch.setattr(ops, "depth_errors", _reference_op)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    scene = str(tmp_path / "scene")
    _write_scene(scene, 14)
    index = str(tmp_path / "index")
    with open(index, "w") as f:
        f.write("00009.png 00006.png 00003.png\n00010.png 00009.png 00006.png\nTRACKING LOST\n00013.png 00010.png 00009.png\n")
    preds, gts, timer = _predict_baseline(_StubBaselineFrame(), scene, index, True, None)
    rows = []
    preds_dev, gts_dev, timer_dev = _predict_baseline(_StubBaselineFrame(static=True), scene, index, True, None, device_evaluate=True,
                                                      error_log=rows)
    assert len(preds) == len(preds_dev) == len(gts) == len(gts_dev) == len(rows) == len(timer_dev.times) == len(timer.times) == 3
    assert not np.array_equal(preds[0], preds[1])            # the stub's static buffer was copied out frame by frame
    for p, g, pd, gd, row in zip(preds, gts, preds_dev, gts_dev, rows):
        assert pd.shape == (256, 320) and np.array_equal(p, pd) and gd.dtype == g.dtype and np.array_equal(g, gd)
        assert row.dtype == np.float32 and row.shape == (8,)
        ref.check_against_host(row, ref.reference(g.astype(np.float32), p)[0], ref.host_errors(g, p))
    assert all(t > 0 for t in timer_dev.times)
    rows = []
    preds, gts, _ = _predict_baseline(_StubBaselineFrame(True), scene, index, False, None, device_evaluate=True, error_log=rows)
    assert len(preds) == 3 and gts is None and rows == []
    shutil.rmtree(os.path.join(scene, "depth"))
    preds, gts, _ = _predict_baseline(_StubBaselineFrame(True), scene, index, True, None, device_evaluate=True, error_log=rows)
    assert len(preds) == 3 and gts is None and rows == []


def test_keyframe_index_reader(tmp_path):
    """Blank lines dropped, ``max_frames`` applied to the stripped lines BEFORE they are parsed (a name the scene does not have, past the
    cut, is never looked up), tracking losses as None, and per line the next keyframe the scene loop of the earlier runner looked for
    with ``next(l for l in lines[n + 1:] if l != "TRACKING LOST")`` -- written out here."""
    from dvmvs.runner import KeyframeIndex
    names = [f"{i:05d}.png" for i in range(8)]
    text = ("\n00003.png 00002.png 00001.png\n  \nTRACKING LOST\nTRACKING LOST\n00004.png 00003.png\n   00005.png 00004.png 00003.png  \n\n"
            "TRACKING LOST\n00007.png 00005.png\nTRACKING LOST\n")
    path = str(tmp_path / "index")
    with open(path, "w") as f:
        f.write(text + "99999.png 00001.png\n")
    lines = [l.strip() for l in text.split("\n") if l.strip()]
    assert len(lines) == 8
    with pytest.raises(KeyError):
        KeyframeIndex(path, names)
    for max_frames in (8, 7, 5, 3, 1, 0):
        index = KeyframeIndex(path, names, max_frames)
        want = lines[:max_frames]
        assert index.lines == want and len(index.frames) == len(index.next_keyframe) == len(want)
        assert index.n_predictions == sum(l != "TRACKING LOST" for l in want)
        for n, line in enumerate(want):
            frames = None if line == "TRACKING LOST" else [int(name[:5]) for name in line.split(" ")]
            assert index.frames[n] == frames
            upcoming = next((l for l in want[n + 1:] if l != "TRACKING LOST"), None)
            found = index.next_keyframe[n]
            assert (want[found] if found is not None else None) == upcoming and (found is None or found > n)
        walked = list(index)
        assert [w[0] for w in walked] == want and [w[1] for w in walked] == index.frames
        assert [w[2] for w in walked] == [index.frames[k] if k is not None else None for k in index.next_keyframe]
    with open(path, "w") as f:
        f.write(text)
    assert KeyframeIndex(path, names).lines == lines and KeyframeIndex(path, names).n_predictions == 4

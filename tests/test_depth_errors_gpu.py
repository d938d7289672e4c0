"""GPU: the depth-evaluation kernel (csrc/depth_errors.hip) on every path -- 16-byte and scalar loads, misaligned frames, ragged sizes, one
and several workgroups, the finishing wave with fewer and more partial sums than lanes, N in {1, 3}, three depth limits, non-finite
predictions -- against the term-exact float64 reference of tests/depth_errors_reference.py (pinned on the CPU by
tests/test_depth_errors_reference.py) within ONE float32 rounding, against the host function by the triangle rule, bit-identical across
calls, batch sizes and alignments, captured in a graph, and through the scene runners with ``device_evaluate=True``."""
import os

import numpy as np
import pytest
import torch

import depth_errors_reference as ref
import synthetic as syn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from dvmvs.hip import ops
    return ops


_references = {}


def _reference(case, N, max_depth):
    """(gt, pred, metrics [N,8], counts [N,4], host rows [N,8]) of a case, computed once and shared (never modified)."""
    key = (case, N, max_depth)
    if key not in _references:
        gt, pred = ref.batch(case, N)
        metrics, counts = ref.reference_batch(gt, pred, max_depth)
        host = np.stack([ref.host_errors(g, p, max_depth) for g, p in zip(gt, pred)])
        _references[key] = (gt, pred, metrics, counts, host)
    return _references[key]


def _at_offset(array, offset, device):
    """``array`` on the device, its first element ``offset`` floats past a 16-byte boundary (a contiguous view into a larger buffer)."""
    buffer = torch.zeros(array.size + offset + 4, dtype=torch.float32, device=device)
    assert buffer.data_ptr() % 16 == 0
    view = buffer[offset:offset + array.size].view(array.shape)
    view.copy_(torch.from_numpy(array))
    assert view.data_ptr() == buffer.data_ptr() + 4 * offset and view.is_contiguous()
    return view


def _check_rows(got, got_counts, metrics, counts, host, what):
    """The rule of the accuracy test.  Counts equal; every finite metric within 2^-23 |ref| of the reference (one float32 rounding of a
    float64 result whose summation error is ~1e-13: derived, not measured); the triangle rule against compute_errors; ratios bit-equal to
    float32(count) / float32(n); NaN / inf where numpy has them."""
    got, got_counts = got.cpu().numpy(), got_counts.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == metrics.shape and np.array_equal(got_counts, counts), (what, got_counts, counts)
    worst = 0.0
    for row, want, c, h in zip(got, metrics, counts, host):
        assert ref.pattern(row) == ref.pattern(want) == ref.pattern(h), (what, row, want, h)
        finite = np.isfinite(want)
        err = np.abs(row[finite].astype(np.float64) - want[finite].astype(np.float64))
        bound = ref.U * np.abs(want[finite].astype(np.float64))
        assert np.all(err <= bound), (what, row, want)
        worst = max(worst, float(np.max(err / np.where(bound > 0, bound, 1.0), initial=0.0)))
        ref.check_against_host(row, want, h)
        if c[0] > 0:
            assert np.array_equal(row[5:], c[1:].astype(np.float32) / np.float32(c[0])), (what, row, c)
    return worst


@pytest.mark.parametrize("case", sorted(ref.CASES))
def test_accuracy_on_every_path(ops, hip_device, case):
    worst = 0.0
    for N in ref.BATCHES:
        for offset in ref.OFFSETS:
            gt, pred = ref.batch(case, N)
            gt_d, pred_d = _at_offset(gt, offset, hip_device), _at_offset(pred, offset, hip_device)
            for max_depth in ref.MAX_DEPTHS:
                _, _, metrics, counts, host = _reference(case, N, max_depth)
                got_counts = torch.full((N, 4), -1, dtype=torch.int32, device=hip_device)
                got = ops.depth_errors(gt_d, pred_d, max_depth=max_depth, counts=got_counts)
                worst = max(worst, _check_rows(got, got_counts, metrics, counts, host, (case, N, offset, max_depth)))
    # the two maps aligned differently: the frame takes the scalar path as a whole
    gt, pred, metrics, counts, host = _reference(case, 1, np.inf)
    got_counts = torch.zeros((1, 4), dtype=torch.int32, device=hip_device)
    got = ops.depth_errors(_at_offset(gt, 0, hip_device), _at_offset(pred, 2, hip_device), counts=got_counts)
    _check_rows(got, got_counts, metrics, counts, host, (case, "mixed alignment"))
    print(f"{case}: max |kernel - reference| = {worst:.2f} * 2^-23 |reference| (bound 1)")


def test_special_cases(ops, hip_device):
    """No valid pixel -> eight NaNs and zero counts; non-finite predictions -> numpy's inf / NaN pattern, finite metrics still within the rule."""
    for what, (gt, pred), max_depth in (("nothing_valid", ref.nothing_valid(), np.inf),
                                        ("all_clipped", ref.frame("ragged_multi"), ref.ALL_CLIPPED_MAX_DEPTH)):
        counts = torch.full((1, 4), -1, dtype=torch.int32, device=hip_device)
        got = ops.depth_errors(torch.from_numpy(gt).to(hip_device), torch.from_numpy(pred).to(hip_device), max_depth=max_depth, counts=counts)
        assert ref.pattern(got.cpu().numpy()[0]) == "n" * 8 == ref.pattern(ref.host_errors(gt, pred, max_depth)), what
        assert not counts.cpu().numpy().any()
    for name, (_, want) in ref.NON_FINITE.items():
        gt, pred = ref.non_finite(name)
        metrics, counts = ref.reference(gt, pred)
        host = ref.host_errors(gt, pred)
        for offset in (0, 1):
            got_counts = torch.zeros((1, 4), dtype=torch.int32, device=hip_device)
            got = ops.depth_errors(_at_offset(gt, offset, hip_device), _at_offset(pred, offset, hip_device), counts=got_counts)
            assert ref.pattern(got.cpu().numpy()[0]) == want, (name, got)
            _check_rows(got, got_counts, metrics[None], counts[None], host[None], name)


@pytest.mark.parametrize("case", ["ragged_multi", "network"])
def test_determinism(ops, hip_device, case):
    """Bit-identical: twice in a row; frame k of a batch of three against the frame alone; at each base offset (load width)."""
    gt, pred = ref.batch(case, 3)
    for max_depth in (np.inf, 2.0):
        rows = []
        for offset in ref.OFFSETS:
            gt_d, pred_d = _at_offset(gt, offset, hip_device), _at_offset(pred, offset, hip_device)
            first = ops.depth_errors(gt_d, pred_d, max_depth=max_depth).cpu().numpy()
            again = ops.depth_errors(gt_d, pred_d, max_depth=max_depth).cpu().numpy()
            assert first.tobytes() == again.tobytes()
            rows.append(first)
            for k in range(3):
                alone = ops.depth_errors(_at_offset(gt[k], offset, hip_device), _at_offset(pred[k], offset, hip_device), max_depth=max_depth)
                assert alone.cpu().numpy()[0].tobytes() == first[k].tobytes(), (case, max_depth, offset, k)
        assert rows[0].tobytes() == rows[1].tobytes() == rows[2].tobytes()


def test_one_launch_and_no_stale_state(ops, hip_device, monkeypatch):
    """A batch is one call into the library and one kernel on the device (no memset, no copy); consecutive calls on the same cached
    workspace each give their own result."""
    from torch.profiler import ProfilerActivity, profile
    from dvmvs.hip import _capi
    lib = _capi.lib()
    calls = []
    real = lib.dvmvs_depth_errors_fwd

    def counted(*args):
        calls.append(args[2])
        return real(*args)

    gt, pred, metrics, counts, host = _reference("half_res", 3, np.inf)
    gt_d, pred_d = torch.from_numpy(gt).to(hip_device), torch.from_numpy(pred).to(hip_device)
    out = torch.empty((3, 8), dtype=torch.float32, device=hip_device)
    ops.depth_errors(gt_d, pred_d, out=out)          # library load, workspace
    torch.cuda.synchronize()
    monkeypatch.setattr(lib, "dvmvs_depth_errors_fwd", counted, raising=False)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        got = ops.depth_errors(gt_d, pred_d, out=out)
        torch.cuda.synchronize()
    monkeypatch.undo()
    activity = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    print("device activity:", activity)
    assert calls == [3] and got.data_ptr() == out.data_ptr()
    assert len(activity) == 1 and "depth_errors_kernel" in activity[0], activity
    # three different inputs through the same workspace (N = 1, half_res): swapped maps, another frame, the first again
    a, b = ref.frame("half_res", 0), ref.frame("half_res", 1)
    workspace = ops.depth_errors_workspace(hip_device, 1, a[0].size)
    for g, p in ((a[0], a[1]), (b[0], b[1]), (a[1], a[0]), (a[0], a[1])):
        want, want_counts = ref.reference(g, p)
        got_counts = torch.zeros((1, 4), dtype=torch.int32, device=hip_device)
        got = ops.depth_errors(torch.from_numpy(g).to(hip_device), torch.from_numpy(p).to(hip_device), counts=got_counts)
        _check_rows(got, got_counts, want[None], want_counts[None], ref.host_errors(g, p)[None], "consecutive")
        assert ops.depth_errors_workspace(hip_device, 1, a[0].size) is workspace
    assert int(workspace.view(torch.int32)[:2].abs().sum()) == 0          # the ticket word is left as it was found


def test_graph_capture(ops, hip_device):
    """depth_errors inside torch.cuda.graph: two replays with changed input contents, both correct."""
    frames = [ref.frame("ragged_multi", k) for k in range(3)]
    gt_d = torch.from_numpy(frames[0][0]).to(hip_device)
    pred_d = torch.from_numpy(frames[0][1]).to(hip_device)
    out = torch.zeros((1, 8), dtype=torch.float32, device=hip_device)
    counts = torch.zeros((1, 4), dtype=torch.int32, device=hip_device)
    ops.depth_errors(gt_d, pred_d, out=out, counts=counts)          # warm-up: the workspace is allocated outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.depth_errors(gt_d, pred_d, out=out, counts=counts)
    for gt, pred in frames[1:]:
        gt_d.copy_(torch.from_numpy(gt))
        pred_d.copy_(torch.from_numpy(pred))
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        want, want_counts = ref.reference(gt, pred)
        _check_rows(out, counts, want[None], want_counts[None], ref.host_errors(gt, pred)[None], "replay")


def test_bad_arguments(ops, hip_device):
    from dvmvs.errors import compute_errors_device
    from dvmvs.hip import _capi
    gt = torch.ones((2, 8, 12), dtype=torch.float32, device=hip_device)
    with pytest.raises(RuntimeError):
        ops.depth_errors(gt.cpu(), gt.cpu())
    with pytest.raises(RuntimeError):
        ops.depth_errors(gt, gt.cpu())
    with pytest.raises(ValueError):
        ops.depth_errors(gt, gt[:, :, :11])
    with pytest.raises(ValueError):
        ops.depth_errors(gt, gt[:1])
    with pytest.raises(ValueError):
        ops.depth_errors(gt.double(), gt.double())
    with pytest.raises(ValueError):
        ops.depth_errors(gt, gt, out=torch.empty((2, 7), device=hip_device))
    with pytest.raises(ValueError):
        ops.depth_errors(gt, gt, counts=torch.empty((2, 4), device=hip_device))
    # the return code alone: sizes the entry point refuses before it touches a pointer (non-null, aligned, never dereferenced)
    lib = _capi.lib()
    inf = float("inf")
    assert lib.dvmvs_depth_errors_fwd(16, 16, 1, 1 << 24, inf, 16, None, 16, None) == -2
    assert lib.dvmvs_depth_errors_fwd(16, 16, 65536, 4, inf, 16, None, 16, None) == -2
    assert lib.dvmvs_depth_errors_fwd(16, 16, 1, 0, inf, 16, None, 16, None) == -1
    assert lib.dvmvs_depth_errors_fwd(None, 16, 1, 4, inf, 16, None, 16, None) == -1
    assert lib.dvmvs_depth_errors_fwd(16, 16, 1, 4, inf, 16, None, None, None) == -1
    assert lib.dvmvs_depth_errors_fwd(16, 16, 1, 4, float("nan"), 16, None, 16, None) == -1
    assert lib.dvmvs_depth_errors_fwd(16, 18, 1, 4, inf, 16, None, 16, None) == -1          # a pointer that is not 4-byte aligned
    assert lib.dvmvs_depth_errors_workspace_bytes(1, 1 << 24) == 0 and lib.dvmvs_depth_errors_workspace_bytes(1, (1 << 24) - 1) > 0
    # the dvmvs.errors spelling: [H,W] -> [8], [N,1,H,W] -> [N,8]
    g, p = ref.frame("sub_wave")
    one = compute_errors_device(torch.from_numpy(g).to(hip_device), torch.from_numpy(p).to(hip_device), max_depth=3.5)
    many = compute_errors_device(torch.from_numpy(g).to(hip_device)[None, None], torch.from_numpy(p).to(hip_device)[None, None], 3.5)
    assert tuple(one.shape) == (8,) and tuple(many.shape) == (1, 8) and one.cpu().numpy().tobytes() == many.cpu().numpy()[0].tobytes()
    assert np.all(np.abs(one.cpu().numpy().astype(np.float64) - ref.reference(g, p, 3.5)[0]) <= ref.U * np.abs(ref.reference(g, p, 3.5)[0]))


# ---- runners: device_evaluate=True against the default path ------------------------------------------------------------------------
def _engine(hip_device):
    from dvmvs.engine import DepthEngine
    from dvmvs.fusionnet.model import CostVolumeDecoder, CostVolumeEncoder, FeatureExtractor, FeatureShrinker, LSTMFusion
    return DepthEngine(*syn.build_e2e_modules((FeatureExtractor, FeatureShrinker, CostVolumeEncoder, LSTMFusion, CostVolumeDecoder)),
                       device=hip_device)


def _check_rows_of_a_run(rows, preds, gts):
    """The rule of the accuracy test against compute_errors on the arrays the runner returned."""
    assert len(rows) == len(preds) == len(gts)
    for row, p, g in zip(rows, preds, gts):
        assert row.dtype == np.float32 and row.shape == (8,)
        want, _ = ref.reference(g.astype(np.float32), p)
        assert np.all(np.abs(row.astype(np.float64) - want) <= ref.U * np.abs(want.astype(np.float64))), (row, want)
        ref.check_against_host(row, want, ref.host_errors(g, p))


def _compare_evaluation_modes(run, what):
    """Each mode gets a fresh engine / network, so both go through the same sequence of eager and replayed frames: identical
    predictions, identical ground truth (same dtype), one metric row per prediction, one positive time per prediction."""
    preds, gts, timer = run(False, None)
    rows = []
    preds_dev, gts_dev, timer_dev = run(True, rows)
    assert len(preds) == len(preds_dev) == len(gts_dev) >= 2 and len(timer.times) == len(preds)
    assert all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(preds, preds_dev))
    assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(gts, gts_dev))
    _check_rows_of_a_run(rows, preds_dev, gts_dev)
    assert len(timer_dev.times) == len(preds_dev) and all(t > 0 for t in timer_dev.times)
    print(f"{what}: {len(preds)} predictions; rows {np.array(rows)[:, 0]}")


@pytest.mark.parametrize("device_preprocess", [False, True])
def test_predict_offline_evaluates_on_the_device(hip_device, tmp_path, device_preprocess):
    from test_runner import _write_scene
    from dvmvs.runner import predict_offline
    scene = os.path.join(str(tmp_path), "scene")
    _write_scene(scene, 14)
    index = os.path.join(str(tmp_path), "index")
    with open(index, "w") as f:
        f.write("00009.png 00006.png 00003.png\n00010.png 00009.png 00006.png\nTRACKING LOST\n00013.png 00010.png 00009.png\n")

    def run(device_evaluate, rows):
        return predict_offline(_engine(hip_device), scene, index, evaluate=True, device_preprocess=device_preprocess,
                               device_evaluate=device_evaluate, error_log=rows)

    _compare_evaluation_modes(run, f"predict_offline(device_preprocess={device_preprocess})")


@pytest.mark.parametrize("device_preprocess", [False, True])
def test_predict_online_evaluates_on_the_device(hip_device, tmp_path, device_preprocess):
    from test_runner import _write_scene
    from dvmvs.runner import predict_online
    scene = os.path.join(str(tmp_path), "scene")
    _write_scene(scene, 16)

    def run(device_evaluate, rows):
        return predict_online(_engine(hip_device), scene, evaluate=True, max_frames=16, device_preprocess=device_preprocess,
                              device_evaluate=device_evaluate, error_log=rows)

    _compare_evaluation_modes(run, f"predict_online(device_preprocess={device_preprocess})")


@pytest.mark.parametrize("device_preprocess", [False, True])
def test_predict_mvdepthnet_evaluates_on_the_device(hip_device, tmp_path, device_preprocess):
    from test_baselines_gpu import _write_scene
    from dvmvs.baselines import runner
    index = _write_scene(str(tmp_path / "scene"))

    def run(device_evaluate, rows):
        return runner.predict_mvdepthnet(str(tmp_path / "scene"), index, device=hip_device, device_preprocess=device_preprocess,
                                         device_evaluate=device_evaluate, error_log=rows)

    _compare_evaluation_modes(run, f"predict_mvdepthnet(device_preprocess={device_preprocess})")


def test_baseline_command_line_switch_and_a_scene_without_ground_truth(hip_device, tmp_path):
    """``python -m dvmvs.baselines.mvdepthnet ... --device-evaluate`` writes the two .npz files of the flagless run: the same predictions,
    error rows within the rule; a scene without depth maps (or evaluate=False) leaves error_log empty and returns None for the depths."""
    import shutil
    from test_baselines_gpu import _write_scene
    from dvmvs.baselines import runner
    index = _write_scene(str(tmp_path / "scene"))
    name = runner.system_name("mvdepthnet", index)
    saved = []
    for flag in ([], ["--device-evaluate"]):
        out = tmp_path / ("out" + str(len(flag)))
        out.mkdir()
        runner.main("mvdepthnet", [str(tmp_path / "scene"), index, "--out", str(out)] + flag)
        assert sorted(os.listdir(out)) == [f"{name}_errors_000.npz", f"{name}_predictions_000.npz"]
        saved.append((np.load(out / f"{name}_predictions_000.npz")["arr_0"], np.load(out / f"{name}_errors_000.npz")["arr_0"]))
    assert saved[0][0].shape == (2, 256, 320) and np.array_equal(saved[0][0], saved[1][0])
    assert saved[0][1].shape == saved[1][1].shape == (2, 8)
    _, gts, _ = runner.predict_mvdepthnet(str(tmp_path / "scene"), index, device=hip_device)
    for host_row, row, p, g in zip(saved[0][1], saved[1][1], saved[1][0], gts):
        assert np.allclose(host_row, ref.host_errors(g, p), rtol=0, atol=0)          # the flagless file holds compute_errors' rows
        ref.check_against_host(row, ref.reference(g.astype(np.float32), p)[0], host_row.astype(np.float64))
    rows = []
    preds, none, timer = runner.predict_mvdepthnet(str(tmp_path / "scene"), index, device=hip_device, evaluate=False, device_evaluate=True,
                                                   error_log=rows)
    assert len(preds) == 2 and none is None and rows == [] and len(timer.times) == 2
    shutil.rmtree(tmp_path / "scene" / "depth")
    preds, none, timer = runner.predict_mvdepthnet(str(tmp_path / "scene"), index, device=hip_device, device_evaluate=True, error_log=rows)
    assert len(preds) == 2 and none is None and rows == [] and np.array_equal(np.stack(preds), saved[0][0])

"""GPU: the RGB SAD sweep (dvmvs::rgb_sweep), GP-MVS's filter step (dvmvs::gp_filter_step) and the MVDepthNet / GP-MVS baselines
end to end against the reference run (tests/golden/baselines_*.npz, make_baseline_goldens.py)."""
import os

import numpy as np
import pytest
import torch

import synthetic as syn
from gp_filter_cpu import gp_filter_step as gp_filter_cpu
from test_baselines import rel_l1, seeded

from dvmvs.baselines import runner
from dvmvs.dataset_loader import PreprocessImage, load_image
from dvmvs.hip import _capi, ops

pytestmark = pytest.mark.gpu


def golden(name):
    return np.load(os.path.join(syn.GOLDEN_DIR, name))


def random_pose(g, behind=False):
    angle = torch.randn(3, generator=g) * (0.05 if not behind else 0.0)
    R = torch.linalg.matrix_exp(torch.tensor([[0.0, -angle[2], angle[1]], [angle[2], 0.0, -angle[0]], [-angle[1], angle[0], 0.0]]))
    if behind:
        R = torch.diag(torch.tensor([-1.0, 1.0, -1.0]))
    pose = torch.eye(4)
    pose[:3, :3] = R
    pose[:3, 3] = torch.randn(3, generator=g) * 0.15 + (torch.tensor([0.0, 0.0, 1.5]) if behind else 0.0)
    return pose


def random_case(B, M, H, W, seed, behind=False):
    g = torch.Generator().manual_seed(seed)
    K = torch.tensor([[0.9 * W, 0.0, W / 2.0], [0.0, 0.9 * W, H / 2.0], [0.0, 0.0, 1.0]]).expand(B, 3, 3).contiguous()
    pose1 = torch.stack([random_pose(g) for _ in range(B)])
    pose2s = [torch.stack([random_pose(g, behind and m == 0) for _ in range(B)]) for m in range(M)]
    from dvmvs.pose_algebra import sweep_matrices_host
    Hm, kt = sweep_matrices_host(pose1, pose2s, K)
    image1 = torch.randn((B, 3, H, W), generator=g)
    image2s = [torch.randn((B, 3, H, W), generator=g) for _ in range(M)]
    return image1, image2s, Hm, kt


def run_sweep(dev, image1, image2s, Hm, kt, D, lo=0.5, hi=50.0, Cout=None, offset=0, copy=False, fill=0.0):
    B, _, H, W = image1.shape
    out = torch.full((B, Cout or D, H, W), fill, device=dev)
    ops.rgb_sweep(out, image1.to(dev), [t.to(dev) for t in image2s], Hm.to(dev), kt.to(dev), lo, hi, D, offset, copy)
    return out


def generic_sad(dev, image1, image2s, Hm, kt, D, lo=0.5, hi=50.0):
    return ops.cost_volume(image1.to(dev), [t.to(dev) for t in image2s], Hm.to(dev), kt.to(dev), lo, hi, D, False, 1)


# ---- RGB sweep ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,M,H,W,D,behind", [(1, 1, 256, 320, 64, False), (1, 2, 256, 320, 64, False), (2, 3, 37, 53, 1, False),
                                              (1, 8, 64, 80, 256, False), (2, 2, 45, 71, 64, True), (1, 3, 129, 161, 64, True)])
def test_rgb_sweep_equals_the_generic_sad_kernel(hip_device, B, M, H, W, D, behind):
    case = random_case(B, M, H, W, seed=B * 1000 + M * 100 + D, behind=behind)
    got = run_sweep(hip_device, *case, D)
    want = generic_sad(hip_device, *case, D)
    diff = (got - want).abs().max().item()
    assert diff == 0.0, f"max |rgb_sweep - generic SAD| = {diff}"


@pytest.mark.parametrize("M", [1, 2])
def test_rgb_sweep_matches_the_reference_on_the_sample_frames(hip_device, M):
    gold = golden("baselines_sad.npz")
    folder = os.path.join(syn.GOLDEN_DIR, "sample_scene", "images")
    K_raw = np.loadtxt(os.path.join(syn.GOLDEN_DIR, "hololens_000_K.txt")).astype(np.float32)
    images = []
    for name in ("00012.png", "00009.png", "00003.png")[:M + 1]:
        raw = load_image(os.path.join(folder, name))
        pre = PreprocessImage(K=K_raw, old_width=raw.shape[1], old_height=raw.shape[0], new_width=320, new_height=256, distortion_crop=0,
                              perform_crop=False)
        images.append(torch.from_numpy(np.ascontiguousarray(np.transpose(pre.apply_rgb(raw, 1.0, [81.0] * 3, [35.0] * 3), (2, 0, 1)))).unsqueeze(0))
    Hm, kt = torch.from_numpy(gold[f"real_M{M}_Hm"]), torch.from_numpy(gold[f"real_M{M}_kt"])
    got = run_sweep(hip_device, images[0], images[1:], Hm, kt, 64).cpu()
    idx = syn.sample_indices(got.numel())
    assert (got.reshape(-1)[idx] - torch.from_numpy(gold[f"real_M{M}_samples"])).abs().max().item() <= 2e-5
    assert abs(got.double().sum().item() - float(gold[f"real_M{M}_sum"])) <= 2e-5 * float(gold[f"real_M{M}_abs_sum"])


@pytest.mark.parametrize("tag", ["behind", "ragged_a", "ragged_b"])
def test_rgb_sweep_matches_the_reference_small_cases(hip_device, tag):
    gold = golden("baselines_sad.npz")
    lo, hi = (float(v) for v in gold[f"{tag}_depth_range"])
    want = torch.from_numpy(gold[f"{tag}_volume"])
    image2s = list(torch.from_numpy(gold[f"{tag}_image2s"]).split(1, 0))
    got = run_sweep(hip_device, torch.from_numpy(gold[f"{tag}_image1"]), image2s, torch.from_numpy(gold[f"{tag}_Hm"]),
                    torch.from_numpy(gold[f"{tag}_kt"]), want.shape[1], lo, hi).cpu()
    assert (got - want).abs().max().item() <= 2e-5


def test_rgb_sweep_fused_slice_copy_and_canary(hip_device):
    B, M, H, W, D = 2, 2, 61, 83, 64
    case = random_case(B, M, H, W, seed=5)
    canary = -12345.0
    volume = run_sweep(hip_device, *case, D)
    # channel slice [3, 67) of a 70-channel buffer, image in 0..2, channels 67..69 untouched
    fused = run_sweep(hip_device, *case, D, Cout=70, offset=3, copy=True, fill=canary)
    assert torch.equal(fused[:, 0:3], case[0].to(hip_device))
    assert torch.equal(fused[:, 3:67], volume)
    assert bool((fused[:, 67:] == canary).all())
    # without copy_image, at an offset: channels outside the slice keep the canary
    sliced = run_sweep(hip_device, *case, D, Cout=D + 9, offset=5, copy=False, fill=canary)
    assert bool((sliced[:, :5] == canary).all()) and bool((sliced[:, 5 + D:] == canary).all())
    assert torch.equal(sliced[:, 5:5 + D], volume)


def test_rgb_sweep_rejects_invalid_arguments_without_a_launch(hip_device):
    lib = _capi.lib()
    dev = hip_device
    x = torch.zeros((1, 3, 16, 16), device=dev)
    out = torch.full((1, 67, 16, 16), 7.0, device=dev)
    Hm, kt = torch.zeros((1, 8, 9), device=dev), torch.zeros((1, 8, 3), device=dev)
    ptrs = _capi.pointer_array([x.data_ptr()] * 9)
    s = torch.cuda.current_stream(dev).cuda_stream
    p = (x.data_ptr(), ptrs, Hm.data_ptr(), kt.data_ptr(), out.data_ptr())
    assert lib.dvmvs_rgb_sweep_fwd(*p, 1, 1, 4, 16, 16, 64, 0.5, 50.0, 67, 3, 1, s) == _capi_unsupported()      # C != 3
    assert lib.dvmvs_rgb_sweep_fwd(*p, 1, 9, 3, 16, 16, 64, 0.5, 50.0, 67, 3, 1, s) == _capi_unsupported()      # M > 8
    assert lib.dvmvs_rgb_sweep_fwd(*p, 1, 1, 3, 16, 16, 257, 0.5, 50.0, 300, 3, 1, s) == _capi_unsupported()   # D > 256
    assert lib.dvmvs_rgb_sweep_fwd(*p, 1, 1, 3, 16, 16, 64, 0.5, 50.0, 66, 3, 1, s) == -1      # slice overruns Cout
    assert lib.dvmvs_rgb_sweep_fwd(*p, 1, 1, 3, 16, 16, 64, 0.5, 50.0, 67, 2, 1, s) == -1      # slice overlaps the image
    assert lib.dvmvs_rgb_sweep_fwd(*p, 1, 1, 3, 16, 16, 64, 0.5, 50.0, 67, -1, 0, s) == -1
    assert lib.dvmvs_rgb_sweep_fwd(None, ptrs, Hm.data_ptr(), kt.data_ptr(), out.data_ptr(), 1, 1, 3, 16, 16, 64, 0.5, 50.0, 67, 3, 1, s) == -1
    assert lib.dvmvs_gp_filter_step(None, x.data_ptr(), x.data_ptr(), 16, 1, 0, 0, 1, 0, 0, 0, s) == -1
    assert lib.dvmvs_gp_filter_step(x.data_ptr(), x.data_ptr(), x.data_ptr(), 0, 1, 0, 0, 1, 0, 0, 0, s) == -1
    torch.cuda.synchronize(dev)
    assert bool((out == 7.0).all())


def _capi_unsupported():
    return -2


# ---- GP filter step -------------------------------------------------------------------------------------------------------
def test_gp_filter_step_matches_numpy_over_20_steps(hip_device):
    rng = np.random.RandomState(3)
    N = 512 * 8 * 10
    state = torch.zeros((2, N), dtype=torch.float64, device=hip_device)
    ref = np.zeros((2, N))
    gp = runner.GPFilter(0.5, 0.3, 0.1)
    for step in range(20):
        y = torch.from_numpy(rng.randn(N).astype(np.float32))
        A, k, reset = gp.step(float(rng.uniform(0.0, 0.5)))
        z = ops.gp_filter_step(state, y.to(hip_device), A, k, reset)
        ref, zref = gp_filter_cpu(ref, y.numpy(), A, k, reset)
        got = state.cpu().numpy()
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
        assert np.array_equal(z.cpu().numpy(), np.maximum(got[0].astype(np.float32), np.float32(0.0)))


# ---- end to end -------------------------------------------------------------------------------------------------------------
def _frames(hip_device, method, monkeypatch):
    """Runs the fixture's five frames (six lines, one TRACKING LOST) through BaselineFrame with the fixture's modules and the fixture
    host's sweep matrices; returns the per-frame depth (and GP-MVS's conv5 / Z)."""
    e2e = golden("baselines_e2e.npz")
    enc = seeded(f"{method}_encoder").to(hip_device)
    dec = seeded(f"{method}_decoder").to(hip_device)
    gp = runner.GPFilter(*(np.float32(v).item() for v in e2e["gp_params"])) if method == "gpmvs" else None
    frame = runner.BaselineFrame(enc, dec, hip_device, gp=gp)
    outs = []
    with torch.no_grad():
        for n in range(int(e2e["n_frames"])):
            r, *ms = (int(v) for v in e2e[f"f{n}_frames"])
            monkeypatch.setattr(runner, "sweep_matrices_host",
                                lambda *a, n=n: (torch.from_numpy(e2e[f"f{n}_Hm"]), torch.from_numpy(e2e[f"f{n}_kt"])))
            rec = {}
            depth = frame(syn.e2e_image(r).to(hip_device), [syn.e2e_image(m).to(hip_device) for m in ms], syn.pose(r),
                          [syn.pose(m) for m in ms], syn.full_K(), dt=float(e2e[f"gp_f{n}_dt"]), outputs=rec)
            outs.append({"depth": depth.cpu(), "conv5": rec["conv5"].cpu(), "Z": rec["Z"].cpu()})
    return e2e, outs


@pytest.mark.parametrize("method", ["mvdepthnet", "gpmvs"])
def test_baseline_depth_matches_the_reference(hip_device, method, monkeypatch):
    e2e, outs = _frames(hip_device, method, monkeypatch)
    prefix = "mv" if method == "mvdepthnet" else "gp"
    for n, o in enumerate(outs):
        err = rel_l1(o["depth"], e2e[f"{prefix}_f{n}_depth_samples"])
        assert err <= 1e-4, f"{method} frame {n}: depth rel-L1 {err:.2e}"
        if method == "gpmvs":
            assert rel_l1(o["conv5"], e2e[f"gp_f{n}_conv5_samples"]) <= 1e-4
            assert rel_l1(o["Z"], e2e[f"gp_f{n}_Z_samples"]) <= 1e-4
    _, again = _frames(hip_device, method, monkeypatch)
    assert all(torch.equal(a["depth"], b["depth"]) for a, b in zip(outs, again)), "two runs differ"


def test_gpmvs_frame_has_no_host_synchronisation(hip_device):
    enc, dec = seeded("gpmvs_encoder").to(hip_device), seeded("gpmvs_decoder").to(hip_device)
    frame = runner.BaselineFrame(enc, dec, hip_device, gp=runner.GPFilter(0.5, 0.3, 0.1))
    ref, meas = syn.e2e_image(9).to(hip_device), [syn.e2e_image(6).to(hip_device), syn.e2e_image(0).to(hip_device)]
    args = (ref, meas, syn.pose(9), [syn.pose(6), syn.pose(0)], syn.full_K())
    with torch.no_grad():
        for _ in range(2):
            frame(*args, dt=0.15)
        torch.cuda.synchronize(hip_device)
        torch.cuda.set_sync_debug_mode("error")
        try:
            depth = frame(*args, dt=0.15)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(depth).all()


# ---- runners ------------------------------------------------------------------------------------------------------------------
def _write_scene(folder):
    os.makedirs(os.path.join(folder, "images"))
    os.makedirs(os.path.join(folder, "depth"))
    src = os.path.join(syn.GOLDEN_DIR, "sample_scene")
    import shutil
    for name in ("00003.png", "00009.png", "00012.png", "00013.png"):
        shutil.copy(os.path.join(src, "images", name), os.path.join(folder, "images", name))
        depth = name if os.path.exists(os.path.join(src, "depth", name)) else "00012.png"
        shutil.copy(os.path.join(src, "depth", depth), os.path.join(folder, "depth", name))
    np.savetxt(os.path.join(folder, "poses.txt"), syn.sample_poses()[[0, 6, 9, 10]].reshape(4, 16))
    np.savetxt(os.path.join(folder, "K.txt"), np.loadtxt(os.path.join(syn.GOLDEN_DIR, "hololens_000_K.txt")))
    index = os.path.join(folder, "keyframe+hololens-dataset+000+nmeas+2")
    with open(index, "w") as f:
        f.write("00012.png 00009.png 00003.png\nTRACKING LOST\n00013.png 00012.png 00009.png\n")
    return index


@pytest.mark.parametrize("method", ["mvdepthnet", "gpmvs"])
def test_runner_on_the_sample_scene(hip_device, tmp_path, method):
    from dvmvs.utils import save_results
    index = _write_scene(str(tmp_path / "scene"))
    predict = runner.predict_mvdepthnet if method == "mvdepthnet" else runner.predict_gpmvs
    predictions, depths, timer = predict(str(tmp_path / "scene"), index, device=hip_device)
    assert len(predictions) == 2 and len(depths) == 2
    assert all(p.shape == (256, 320) and np.isfinite(p).all() and p.min() >= 0.5 - 1e-6 and p.max() <= 50.0 + 1e-4 for p in predictions)
    name = runner.system_name(method, index)
    assert name == f"keyframe_hololens-dataset_320_256_2_{method}_finetuned"
    out = tmp_path / "out"
    out.mkdir()
    save_results(predictions, depths, name, "000", str(out))
    assert sorted(os.listdir(out)) == [f"{name}_errors_000.npz", f"{name}_predictions_000.npz"]
    saved = np.load(out / f"{name}_predictions_000.npz")
    assert list(saved.keys()) == ["arr_0"] and saved["arr_0"].shape == (2, 256, 320)
    assert np.load(out / f"{name}_errors_000.npz")["arr_0"].shape == (2, 8)


class ModeRuns:
    """One predict_* entry point on one scene under the (device_preprocess, device_evaluate) combinations: each combination is run once
    (a fresh network per run, as the entry points build it), kept, and compared read-only."""

    def __init__(self, predict, scene, index, device, **keywords):
        self.predict, self.scene, self.index, self.device, self.keywords = predict, scene, index, device, keywords
        self.done = {}

    def __call__(self, device_preprocess, device_evaluate):
        """(predictions, ground truths, timer, error rows)"""
        mode = (bool(device_preprocess), bool(device_evaluate))
        if mode not in self.done:
            rows = []
            self.done[mode] = self.predict(self.scene, self.index, device=self.device, device_preprocess=mode[0], device_evaluate=mode[1],
                                           error_log=rows, **self.keywords) + (rows,)
        return self.done[mode]

    def check(self, device_preprocess, device_evaluate, what):
        """Against the default call: tests/test_preprocess_gpu.py's rule wherever device_preprocess is set, tests/test_depth_errors_gpu.py's
        wherever device_evaluate is (its two runs share ``device_preprocess``: it asks for the ground truth's dtype to stay)."""
        from test_depth_errors_gpu import _compare_evaluation_modes
        from test_preprocess_gpu import _compare_modes
        what = f"{what}(device_preprocess={device_preprocess}, device_evaluate={device_evaluate})"
        assert len(self(False, False)[0]) == 2 and self(False, False)[3] == []
        if device_preprocess:
            _compare_modes(lambda flag, log: self(flag, flag and device_evaluate)[:2], what)
        if device_evaluate:
            def run(flag, rows):
                if rows is not None:
                    rows.extend(self(device_preprocess, flag)[3])
                return self(device_preprocess, flag)[:3]
            _compare_evaluation_modes(run, what)


@pytest.fixture(scope="module")
def gpmvs_runs(hip_device, tmp_path_factory):
    scene = str(tmp_path_factory.mktemp("gpmvs") / "scene")
    return ModeRuns(runner.predict_gpmvs, scene, _write_scene(scene), hip_device)


@pytest.mark.parametrize("device_preprocess,device_evaluate", [(True, False), (False, True), (True, True)])
def test_predict_gpmvs_in_every_mode(gpmvs_runs, device_preprocess, device_evaluate):
    gpmvs_runs.check(device_preprocess, device_evaluate, "predict_gpmvs")

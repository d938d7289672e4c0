"""GPU: the DPSNet plane volume (dvmvs::dps_volume), the up-sampling soft-argmin (dvmvs::dps_regress) and the baseline end to end
against the reference run (tests/golden/dpsnet_*.npz, make_dpsnet_goldens.py).  Reads only tests/golden.

Bounds.  Plane volume: against the float64 evaluation of the reference's expressions, 4x the reference's own fp32 error against it
(recorded per case by the generator), the elements whose un-masked coordinate lies within 1e-4 of +-1 left out (at most 0.1 % of a
case).  Regression: 4x the error of the reference's fp32 chain on pred, and 4x that chain's relative error on the depth where
pred >= 0.5.  End to end: rel-L1 <= 1e-4 on pred0 and pred against the reference pins."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dpsnet_fixtures as fx
import synthetic as syn
from test_dpsnet import (E2E_BOUND, check_regress, check_volume, e2e_errors, e2e_inputs, regress_cases, regress_inputs, volume_cases,
                         volume_inputs)

from dvmvs.baselines import runner
from dvmvs.baselines.dpsnet.dpsnet import PSNet
from dvmvs.hip import _capi, ops

pytestmark = pytest.mark.gpu


# ---- plane volume ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", volume_cases())
def test_dps_volume_matches_the_reference(hip_device, tag):
    ref, meas, pose, K4, Kinv4, nlabel = volume_inputs(tag)
    args = [t.to(hip_device) for t in (ref, meas, pose, K4, Kinv4)]
    volume = ops.dps_volume(*args, nlabel, fx.MINDEPTH)
    assert tuple(volume.shape) == (ref.shape[0], 2 * ref.shape[1], nlabel, ref.shape[2], ref.shape[3])
    check_volume(tag, ref, volume)
    assert torch.equal(volume, ops.dps_volume(*args, nlabel, fx.MINDEPTH)), "two runs differ"


def test_dps_volume_writes_nothing_outside_its_output(hip_device):
    """The C entry point on a buffer with a canary on either side: ragged sizes, B = 2."""
    tag = fx.VOLUME_SMALL[1][0]
    ref, meas, pose, K4, Kinv4, nlabel = (t.to(hip_device) if isinstance(t, torch.Tensor) else t for t in volume_inputs(tag))
    B, C, h, w = ref.shape
    n = B * 2 * C * nlabel * h * w
    pad, canary = 4096, -12345.0
    buffer = torch.full((n + 2 * pad,), canary, device=hip_device)
    out = buffer[pad:pad + n]
    rc = _capi.lib().dvmvs_dps_volume_fwd(ref.data_ptr(), meas.data_ptr(), pose.data_ptr(), K4.data_ptr(), Kinv4.data_ptr(), out.data_ptr(),
                                          B, C, h, w, nlabel, fx.MINDEPTH, torch.cuda.current_stream(hip_device).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize(hip_device)
    assert bool((buffer[:pad] == canary).all()) and bool((buffer[pad + n:] == canary).all())
    assert torch.equal(out.view(B, 2 * C, nlabel, h, w), ops.dps_volume(ref, meas, pose, K4, Kinv4, nlabel, fx.MINDEPTH))
    check_volume(tag, ref.cpu(), out.view(B, 2 * C, nlabel, h, w))


def test_entry_points_reject_invalid_arguments_without_a_launch(hip_device):
    lib = _capi.lib()
    x = torch.full((4096,), 7.0, device=hip_device)
    p, s = x.data_ptr(), torch.cuda.current_stream(hip_device).cuda_stream
    assert lib.dvmvs_dps_volume_fwd(p, p, p, p, p, p, 1, 65, 4, 4, 4, 0.5, s) == -2
    assert lib.dvmvs_dps_volume_fwd(p, p, p, p, p, p, 1, 4, 4, 4, 257, 0.5, s) == -2
    assert lib.dvmvs_dps_volume_fwd(p, p, None, p, p, p, 1, 4, 4, 4, 4, 0.5, s) == -1
    assert lib.dvmvs_dps_regress_fwd(p, p, p, 1, 257, 4, 4, 8, 8, 0.5, s) == -2
    assert lib.dvmvs_dps_regress_fwd(p, p, p, 1, 4, 4, 4, 8, -8, 0.5, s) == -1
    torch.cuda.synchronize(hip_device)
    assert bool((x == 7.0).all())
    with pytest.raises(RuntimeError):
        ops.dps_volume(torch.zeros(1, 4, 4, 4), torch.zeros(1, 4, 4, 4), torch.zeros(1, 3, 4), torch.eye(3)[None], torch.eye(3)[None], 4, 0.5)


# ---- regression --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,kind", regress_cases())
def test_dps_regress_matches_the_reference(hip_device, size, kind):
    costs, H, W = regress_inputs(size, kind)
    depth, pred = ops.dps_regress(costs.to(hip_device), H, W, fx.MINDEPTH)
    assert tuple(depth.shape) == (1, 1, H, W) and tuple(pred.shape) == (1, H, W)
    check_regress(size, kind, pred, depth)
    again = ops.dps_regress(costs[:, 0].to(hip_device), H, W, fx.MINDEPTH)          # [B,nlabel,h,w] is accepted too
    assert torch.equal(again[0], depth) and torch.equal(again[1], pred), "two runs differ"


def test_dps_regress_accepts_a_null_pred_pointer_and_a_batch(hip_device):
    costs = torch.cat([regress_inputs("ragged", "random")[0], regress_inputs("ragged", "peak")[0]], 0).to(hip_device)
    _, H, W = regress_inputs("ragged", "random")
    depth, pred = ops.dps_regress(costs, H, W, fx.MINDEPTH)
    only_depth, empty = ops.dps_regress(costs, H, W, fx.MINDEPTH, False)
    assert empty.numel() == 0 and torch.equal(only_depth, depth)
    for b, kind in enumerate(("random", "peak")):
        check_regress("ragged", kind, pred[b:b + 1], depth[b:b + 1])
    # the C entry point with pred = null and a canary behind the depth buffer
    n = depth.numel()
    buffer = torch.full((n + 1024,), -7.0, device=hip_device)
    rc = _capi.lib().dvmvs_dps_regress_fwd(costs.data_ptr(), buffer.data_ptr(), None, costs.shape[0], costs.shape[2], costs.shape[3], costs.shape[4],
                                           H, W, fx.MINDEPTH, torch.cuda.current_stream(hip_device).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize(hip_device)
    assert torch.equal(buffer[:n].view_as(depth), depth) and bool((buffer[n:] == -7.0).all())


def test_dps_regress_interpolates_the_costs_not_the_probabilities(hip_device):
    """Two neighbouring source pixels with their peaks on different planes: half-way between them the up-sampled COSTS have two equal
    peaks of half the height above a flat floor, so the expectation is pulled towards the floor's mean; up-sampled PROBABILITIES
    would give the mean of the two peak planes."""
    nlabel, h, w, H, W = 64, 2, 2, 8, 8
    costs = torch.zeros((1, 1, nlabel, h, w))
    costs[0, 0, 2, :, 0] = 4.0
    costs[0, 0, 60, :, 1] = 4.0
    up = F.interpolate(costs.double(), [nlabel, H, W], mode="trilinear", align_corners=False)[:, 0]
    planes = torch.arange(nlabel, dtype=torch.float64).view(1, nlabel, 1, 1)
    costs_first = (F.softmax(up, 1) * planes).sum(1)
    probs_first = (F.interpolate(F.softmax(costs.double(), 2), [nlabel, H, W], mode="trilinear", align_corners=False)[:, 0] * planes).sum(1)
    assert (costs_first - probs_first).abs().max().item() > 0.2          # the case separates the two orders
    _, pred = ops.dps_regress(costs.to(hip_device), H, W, 0.5)
    pred = pred.cpu().double()
    assert (pred - costs_first).abs().max().item() <= 1e-4
    assert (pred - probs_first).abs().max().item() > 0.2


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------
def _run_frames(net, hip_device, tags):
    outs = []
    with torch.no_grad():
        for tag in tags:
            out = {}
            depth0, depth = net(*e2e_inputs(tag, hip_device), outputs=out)
            out.update(depth0=depth0, depth=depth)
            outs.append({k: v.cpu() for k, v in out.items()})
    return outs


def test_dpsnet_matches_the_reference_end_to_end(hip_device):
    e2e = fx.golden("dpsnet_e2e.npz")
    net = fx.seeded_dpsnet(PSNet).to(hip_device)
    tags = [f"f{n}" for n in range(int(e2e["n_frames"]))] + ["small"]
    outs = _run_frames(net, hip_device, tags)
    for tag, out in zip(tags, outs):
        errors = e2e_errors(tag, out, ("features", "costs", "costss", "pred0", "pred"))
        assert errors["pred0"] <= E2E_BOUND and errors["pred"] <= E2E_BOUND, f"{tag}: {errors}"
        idx = syn.sample_indices(out["pred"].numel())
        keep = torch.from_numpy(e2e[f"{tag}_pred_samples"]) >= 0.5
        want = torch.from_numpy(e2e[f"{tag}_depth_samples"]).double()[keep]
        got = out["depth"].reshape(-1)[idx].double()[keep]
        assert ((got - want).abs().sum() / want.abs().sum()).item() <= E2E_BOUND, f"{tag}: depth"
        assert tuple(out["depth"].shape) == (1, 1, *out["pred"].shape[1:])
    again = _run_frames(net, hip_device, tags)
    assert all(torch.equal(a["depth"], b["depth"]) and torch.equal(a["depth0"], b["depth0"]) for a, b in zip(outs, again)), "two runs differ"


def test_fused_route_against_the_plain_route_on_the_device(hip_device):
    """The reference's formulation with the same tensors on the device (per-plane volume, per-plane context network, materialised
    up-sampling) against the fused route."""
    net = fx.seeded_dpsnet(PSNet).to(hip_device)
    inputs = e2e_inputs("small", hip_device)
    fused, plain = {}, {}
    with torch.no_grad():
        net.route = "fused"
        net(*inputs, outputs=fused)
        net.route = "plain"
        net(*inputs, outputs=plain)
    for key in ("costs", "costss", "pred0", "pred"):
        err = ((fused[key] - plain[key]).abs().sum() / plain[key].abs().sum()).item()
        print(f"fused vs plain on the device, {key}: rel-L1 {err:.2e}")
        assert err <= E2E_BOUND, key
    print("plain route on the device against the reference pins:")
    e2e_errors("small", {k: v.cpu() for k, v in plain.items()}, ("costs", "costss", "pred0", "pred"))


def test_batched_context_network_equals_the_per_plane_loop(hip_device):
    e2e = fx.golden("dpsnet_e2e.npz")
    net = fx.seeded_dpsnet(PSNet).to(hip_device)
    out = {}
    with torch.no_grad():
        net(*e2e_inputs("f0", hip_device), outputs=out)
        per_plane = net.context_per_plane(out["features"], out["costs"])
    assert per_plane.shape == out["costss"].shape
    err = ((out["costss"] - per_plane).abs().sum() / per_plane.abs().sum()).item()
    assert err <= E2E_BOUND, f"batched vs per-plane context network: rel-L1 {err:.2e}"
    assert fx.rel_l1(per_plane.cpu(), e2e["f0_costss_samples"]) <= E2E_BOUND


def test_frame_has_no_host_synchronisation(hip_device):
    net = fx.seeded_dpsnet(PSNet).to(hip_device)
    inputs = e2e_inputs("f0", hip_device)
    with torch.no_grad():
        for _ in range(2):
            net(*inputs)
        torch.cuda.synchronize(hip_device)
        torch.cuda.set_sync_debug_mode("error")
        try:
            _, depth = net(*inputs)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(depth).all()


def test_cuda_inference_takes_the_fused_route(hip_device, monkeypatch):
    """No silent fallback: with the kernel taken away, CUDA inference raises instead of running eager PyTorch."""
    net = PSNet(4, 0.5).to(hip_device).eval()
    K = torch.tensor([[[120.0, 0.0, 64.0], [0.0, 120.0, 64.0], [0.0, 0.0, 1.0]]], device=hip_device)
    pose = torch.eye(4, device=hip_device)[:3].unsqueeze(0)
    image = torch.randn((1, 3, 128, 128), device=hip_device)

    def missing(*args, **kwargs):
        raise RuntimeError("dvmvs HIP library not found")

    monkeypatch.setattr(ops, "dps_volume", missing)
    with torch.no_grad(), pytest.raises(RuntimeError, match="not found"):
        net(image, [image], [pose], K, torch.inverse(K))


# ---- runner ------------------------------------------------------------------------------------------------------------------------------
def _write_scene(folder):
    import shutil
    os.makedirs(os.path.join(folder, "images"))
    os.makedirs(os.path.join(folder, "depth"))
    src = os.path.join(syn.GOLDEN_DIR, "sample_scene")
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


def test_runner_on_the_sample_scene(hip_device, tmp_path):
    from dvmvs.utils import save_results
    index = _write_scene(str(tmp_path / "scene"))
    predictions, depths, timer = runner.predict_dpsnet(str(tmp_path / "scene"), index, device=hip_device)
    assert len(predictions) == 2 and len(depths) == 2
    assert all(p.shape == (240, 320) and np.isfinite(p).all() for p in predictions)
    assert all(d.shape == (240, 320) for d in depths)
    name = runner.system_name("dpsnet", index, size=(runner.DPS_WIDTH, runner.DPS_HEIGHT))
    assert name == "keyframe_hololens-dataset_320_240_2_dpsnet_finetuned"
    out = tmp_path / "out"
    out.mkdir()
    save_results(predictions, depths, name, "000", str(out))
    assert sorted(os.listdir(out)) == [f"{name}_errors_000.npz", f"{name}_predictions_000.npz"]
    assert np.load(out / f"{name}_predictions_000.npz")["arr_0"].shape == (2, 240, 320)


@pytest.fixture(scope="module")
def dpsnet_runs(hip_device, tmp_path_factory):
    """predict_dpsnet with the fixtures' network (dpsnet_fixtures.seeded_dpsnet, loaded as a ``*dpsnet*`` checkpoint), not the default
    initialisation: that one saturates the soft-argmin -- the disparity sits at its 1e-16 clamp and the "depth" is 32 / 1e-16 = 3.2e17 on
    most pixels -- which is the case the fixtures' factors exist to avoid, and no depth map: compute_errors on float32 maps is defined
    only while the sum of the squared differences stays below float32's 3.4e38, i.e. below 6.6e16 per pixel over 320 x 240 pixels."""
    from test_baselines_gpu import ModeRuns
    folder = tmp_path_factory.mktemp("dpsnet")
    torch.save(fx.seeded_dpsnet(PSNet).state_dict(), str(folder / "dpsnet_fixture_weights"))
    scene = str(folder / "scene")
    return ModeRuns(runner.predict_dpsnet, scene, _write_scene(scene), hip_device, weights_folder=str(folder))


@pytest.mark.parametrize("device_preprocess,device_evaluate", [(True, False), (False, True), (True, True)])
def test_predict_dpsnet_in_every_mode(dpsnet_runs, device_preprocess, device_evaluate):
    dpsnet_runs.check(device_preprocess, device_evaluate, "predict_dpsnet")
    assert all(np.isfinite(p).all() and p.max() < 6.6e16 for p in dpsnet_runs(False, False)[0])

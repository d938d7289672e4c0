"""CPU: the DPSNet baseline (dvmvs.baselines.dpsnet) against the reference's module surface, and its plain-torch route against the
fixtures of the reference run (tests/golden/dpsnet_*.npz, make_dpsnet_goldens.py).  The fused route is tested on the GPU
(test_dpsnet_gpu.py) with the same comparisons, which live here."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import dpsnet_fixtures as fx
import synthetic as syn

from dvmvs.baselines import runner
from dvmvs.baselines.dpsnet import dpsnet as dps
from dvmvs.baselines.dpsnet.dpsnet import PSNet

NEAR_MASK_CAP = 1e-3        # at most 0.1 % of a case's elements may be left out as "near the mask"
E2E_BOUND = 1e-4            # the project's bound for every end-to-end pin (rel-L1)


# ---- comparisons shared with the GPU tests -----------------------------------------------------------------------------------------
def volume_cases():
    return [f"pair{n}" for n in range(len(fx.VOLUME_PAIRS))] + [c[0] for c in fx.VOLUME_SMALL]


def volume_inputs(tag):
    """(ref, meas, pose, K4, Kinv4, nlabel) of a case of dpsnet_volume.npz, rebuilt from seeds and the fixture's matrices."""
    gold = fx.golden("dpsnet_volume.npz")
    if tag.startswith("pair"):
        n = int(tag[4:])
        ref, meas = fx.feature_maps(1, 32, 60, 80, seed=300 + 2 * n)
        nlabel = fx.NLABEL
    else:
        n = [c[0] for c in fx.VOLUME_SMALL].index(tag)
        _, B, C, nlabel, h, w, _ = fx.VOLUME_SMALL[n]
        ref, meas = fx.feature_maps(B, C, h, w, seed=400 + 2 * n)
    return ref, meas, torch.from_numpy(gold[f"{tag}_pose"]), torch.from_numpy(gold[f"{tag}_K4"]), torch.from_numpy(gold[f"{tag}_Kinv4"]), nlabel


def check_volume(tag, ref, volume):
    """``volume`` [B,2C,nlabel,h,w] against the case: the first half bit-equal to the reference features; the warped half within 4x the
    reference's own fp32 error of the float64 evaluation, the elements near the mask (at most 0.1 %) left out.  Returns the error."""
    gold = fx.golden("dpsnet_volume.npz")
    volume = volume.detach().cpu()
    B, C2, nlabel, h, w = volume.shape
    C = C2 // 2
    assert torch.equal(volume[:, :C], ref.unsqueeze(2).expand(B, C, nlabel, h, w)), f"{tag}: reference half differs"
    warped = volume[:, C:].contiguous()
    near_pixels = torch.zeros(B * nlabel * h * w, dtype=torch.bool)
    near_pixels[torch.from_numpy(gold[f"{tag}_near"]).long()] = True
    near = near_pixels.view(B, 1, nlabel, h, w).expand(B, C, nlabel, h, w).reshape(-1)
    share = near.float().mean().item()
    assert share <= NEAR_MASK_CAP, f"{tag}: {share:.2e} of the elements lie near the mask"
    bound = 4.0 * float(gold[f"{tag}_ref_err"])
    if f"{tag}_warped64" in gold.files:
        want, got, skip = torch.from_numpy(gold[f"{tag}_warped64"]).reshape(-1), warped.reshape(-1), near
    else:
        idx = syn.sample_indices(warped.numel(), fx.VOLUME_PIN_COUNT)
        want, got, skip = torch.from_numpy(gold[f"{tag}_samples64"]), warped.reshape(-1)[idx], near[idx]
    err = ((got.double() - want).abs() * (~skip)).max().item()
    print(f"{tag}: max |volume - float64| {err:.3e} (bound {bound:.3e}, reference fp32 {float(gold[f'{tag}_ref_err']):.3e}), "
          f"near the mask {share:.2e}")
    assert err <= bound, f"{tag}: max |volume - float64| {err:.3e} > {bound:.3e}"
    return err


def regress_cases():
    return [(size[0], kind) for size in fx.REGRESS_SIZES for kind in fx.REGRESS_KINDS]


def regress_inputs(size, kind):
    s = [c[0] for c in fx.REGRESS_SIZES].index(size)
    _, nlabel, h, w, H, W = fx.REGRESS_SIZES[s]
    return fx.regress_costs(kind, nlabel, h, w, seed=500 + 10 * s + fx.REGRESS_KINDS.index(kind)), H, W


def check_regress(size, kind, pred, depth):
    """pred [B,H,W] within 4x the error of the reference's fp32 chain against float64; depth, where pred >= 0.5, within 4x that chain's
    relative error on the depth (the same chain's error, carried through the reciprocal); everything finite."""
    gold = fx.golden("dpsnet_regress.npz")
    tag = f"{size}_{kind}"
    pred, depth = pred.detach().cpu(), depth.detach().cpu()
    assert torch.isfinite(pred).all() and torch.isfinite(depth).all(), f"{tag}: not finite"
    if f"{tag}_pred64" in gold.files:
        p, d = pred.reshape(-1), depth.reshape(-1)
        p64, d64 = torch.from_numpy(gold[f"{tag}_pred64"]).reshape(-1), torch.from_numpy(gold[f"{tag}_depth64"]).reshape(-1)
    else:
        idx = syn.sample_indices(pred.numel(), fx.REGRESS_PIN_COUNT)
        p, d = pred.reshape(-1)[idx], depth.reshape(-1)[idx]
        p64, d64 = torch.from_numpy(gold[f"{tag}_pred64_samples"]), torch.from_numpy(gold[f"{tag}_depth64_samples"])
    err = (p.double() - p64).abs().max().item()
    ok = p64 >= 0.5
    rel = (((d.double() - d64).abs() / d64)[ok]).max().item() if ok.any() else 0.0
    print(f"{tag}: max |pred - float64| {err:.3e} (reference fp32 {float(gold[f'{tag}_pred_err']):.3e}), depth rel {rel:.3e} "
          f"(reference fp32 {float(gold[f'{tag}_depth_rel_err']):.3e})")
    assert err <= 4.0 * float(gold[f"{tag}_pred_err"]), f"{tag}: pred error {err:.3e}"
    assert rel <= 4.0 * float(gold[f"{tag}_depth_rel_err"]), f"{tag}: depth relative error {rel:.3e}"


def e2e_inputs(tag, device="cpu"):
    """(ref, targets, poses, K, Kinv) of a frame of dpsnet_e2e.npz."""
    e2e = fx.golden("dpsnet_e2e.npz")
    r, *ms = (int(v) for v in e2e[f"{tag}_frames"])
    H, W = fx.E2E_SMALL if tag == "small" else (240, 320)
    poses = torch.from_numpy(e2e[f"{tag}_poses"])
    return (fx.e2e_image(r, H, W).to(device), [fx.e2e_image(m, H, W).to(device) for m in ms], [poses[j:j + 1].to(device) for j in range(len(ms))],
            torch.from_numpy(e2e[f"{tag}_K"]).to(device), torch.from_numpy(e2e[f"{tag}_Kinv"]).to(device))


def e2e_errors(tag, outputs, keys):
    e2e = fx.golden("dpsnet_e2e.npz")
    errors = {key: fx.rel_l1(outputs[key], e2e[f"{tag}_{key}_samples"]) for key in keys}
    print(f"{tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in errors.items()))
    return errors


# ---- module surface ------------------------------------------------------------------------------------------------------------------
def test_state_dict_keys_and_shapes_match_the_reference(tmp_path):
    with open(os.path.join(syn.GOLDEN_DIR, "dpsnet_state_dict_keys.json")) as f:
        expected = json.load(f)
    net = PSNet(fx.NLABEL, fx.MINDEPTH)
    assert len(expected) == 435
    assert {k: list(v.shape) for k, v in net.state_dict().items()} == expected
    assert sum(p.numel() for p in net.parameters()) == 4190432
    # a checkpoint written from the fixture's key list alone loads strictly, plain and as {'state_dict': ...}
    state = {k: torch.full(shape, 0.25) if k.split(".")[-1] != "num_batches_tracked" else torch.tensor(3) for k, shape in expected.items()}
    net.load_state_dict(state, strict=True)
    for name, checkpoint in (("plain", state), ("wrapped", {"state_dict": state, "epoch": 1})):
        folder = tmp_path / name
        folder.mkdir()
        torch.save(checkpoint, folder / "finetuned_dpsnet")
        loaded = runner.build_dpsnet(folder, device="cpu", seed=3)
        assert not loaded.training and all(torch.equal(v, state[k]) for k, v in loaded.state_dict().items())


def test_reference_helper_names_exist():
    for name in ("inverse_warp", "convbn", "convbn_3d", "BasicBlock", "convtext", "disparityregression", "feature_extraction", "PSNet"):
        assert hasattr(dps, name), name
    assert not hasattr(dps, "pixel_coords")
    assert isinstance(dps.convbn_3d(4, 4, 3, 1, 1)[1], torch.nn.BatchNorm3d)


def test_same_seed_same_initialisation():
    torch.manual_seed(4)
    a = PSNet(8, 0.5).state_dict()
    torch.manual_seed(4)
    b = PSNet(8, 0.5).state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    w = a["dres0.0.0.weight"]          # normal(0, sqrt(2 / (27 * 32)))
    assert abs(w.std().item() / (2.0 / (27 * 32)) ** 0.5 - 1.0) < 0.05 and a["dres0.0.1.weight"].eq(1).all()


def test_train_keeps_batchnorm_frozen():
    net = PSNet(fx.NLABEL, fx.MINDEPTH)
    assert net.train() is net
    bns = [m for m in net.modules() if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.BatchNorm3d))]
    # 60 two-dimensional layers in the feature extractor, 11 three-dimensional ones in dres0..4 and classify
    assert net.training and len(bns) == 71 and all(not m.training and not m.weight.requires_grad and not m.bias.requires_grad for m in bns)
    assert any(isinstance(m, torch.nn.BatchNorm3d) for m in bns)


def test_system_names():
    f = "keyframe+hololens-dataset+000+nmeas+2"
    assert runner.system_name("mvdepthnet", f) == "keyframe_hololens-dataset_320_256_2_mvdepthnet_finetuned"
    assert runner.system_name("gpmvs", "/x/" + f, finetuned=False) == "keyframe_hololens-dataset_320_256_2_gpmvs_without_ft"
    assert runner.system_name("dpsnet", f, size=(runner.DPS_WIDTH, runner.DPS_HEIGHT)) == "keyframe_hololens-dataset_320_240_2_dpsnet_finetuned"
    assert runner.system_name("dpsnet", f, False, (320, 240)) == "keyframe_hololens-dataset_320_240_2_dpsnet_without_ft"


def test_runner_relative_pose_is_float64_then_cast():
    poses = syn.sample_poses()
    got = runner.dpsnet_relative_pose(poses[9], poses[6])
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, 3, 4) and torch.equal(got, fx.relative_pose(9, 6))


# ---- plain-torch route against the fixtures ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", volume_cases())
def test_plain_volume_matches_the_reference(tag):
    ref, meas, pose, K4, Kinv4, nlabel = volume_inputs(tag)
    net = PSNet(nlabel, fx.MINDEPTH)
    with torch.no_grad():
        volume = net.plane_volume(ref, meas, pose, K4, Kinv4)
    check_volume(tag, ref, volume)


@pytest.mark.parametrize("size,kind", regress_cases())
def test_plain_regression_matches_the_reference(size, kind):
    costs, H, W = regress_inputs(size, kind)
    net = PSNet(costs.shape[2], fx.MINDEPTH)
    depth, pred = net.regress(costs, H, W)
    assert tuple(depth.shape) == (1, 1, H, W) and tuple(pred.shape) == (1, H, W)
    check_regress(size, kind, pred, depth)


def test_plain_route_matches_the_reference_on_the_small_frame():
    net = fx.seeded_dpsnet(PSNet)
    out = {}
    with torch.no_grad():
        depth0, depth = net(*e2e_inputs("small"), outputs=out)
    out.update(depth0=depth0, depth=depth)
    errors = e2e_errors("small", out, ("features", "costs", "costss", "pred0", "pred", "depth0", "depth"))
    assert all(v <= E2E_BOUND for v in errors.values()), errors
    # the fixture's own condition on the seeded module: the soft-argmin is not stuck at plane 0
    assert (out["pred"] < 0.5).float().mean().item() < 0.05


def test_batched_context_network_equals_the_per_plane_loop_on_cpu():
    net = fx.seeded_dpsnet(PSNet)
    g = torch.Generator().manual_seed(1)
    fea, costs = torch.randn((2, 32, 9, 12), generator=g), torch.randn((2, 1, fx.NLABEL, 9, 12), generator=g)
    with torch.no_grad():
        a, b = net.context_batched(fea, costs), net.context_per_plane(fea, costs)
    assert a.shape == b.shape and (a - b).abs().max().item() <= 1e-5 * b.abs().max().item()


def test_gradients_take_the_plain_route():
    net = PSNet(4, 0.5).eval()
    ref = torch.randn((1, 3, 128, 128), requires_grad=True)
    K = torch.tensor([[[120.0, 0.0, 64.0], [0.0, 120.0, 64.0], [0.0, 0.0, 1.0]]])
    pose = torch.eye(4)[:3].unsqueeze(0).clone()
    pose[0, 0, 3] = 0.1
    _, depth = net(ref, [torch.randn((1, 3, 128, 128))], [pose], K, torch.inverse(K))
    depth.sum().backward()
    assert ref.grad is not None and torch.isfinite(ref.grad).all()


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_entry_points_validate_arguments_without_a_device():
    """Negative return codes come before anything is enqueued, so fake non-null pointers are never dereferenced."""
    from dvmvs.hip import _capi
    lib = _capi.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert lib.dvmvs_dps_volume_fwd(None, p, p, p, p, p, 1, 32, 60, 80, 64, 0.5, None) == -1
    assert lib.dvmvs_dps_volume_fwd(p, p, p, p, p, None, 1, 32, 60, 80, 64, 0.5, None) == -1
    assert lib.dvmvs_dps_volume_fwd(p, p, p, p, p, p, 0, 32, 60, 80, 64, 0.5, None) == -1
    assert lib.dvmvs_dps_volume_fwd(p, p, p, p, p, p, 1, 32, 60, 80, 64, 0.0, None) == -1
    assert lib.dvmvs_dps_volume_fwd(p, p, p, p, p, p, 1, 65, 60, 80, 64, 0.5, None) == -2
    assert lib.dvmvs_dps_volume_fwd(p, p, p, p, p, p, 1, 32, 60, 80, 257, 0.5, None) == -2
    assert lib.dvmvs_dps_regress_fwd(None, p, p, 1, 64, 60, 80, 240, 320, 0.5, None) == -1
    assert lib.dvmvs_dps_regress_fwd(p, None, p, 1, 64, 60, 80, 240, 320, 0.5, None) == -1
    assert lib.dvmvs_dps_regress_fwd(p, p, None, 1, 64, 60, 80, 0, 320, 0.5, None) == -1
    assert lib.dvmvs_dps_regress_fwd(p, p, None, 1, 257, 60, 80, 240, 320, 0.5, None) == -2
    assert _capi.ABI_VERSION == 11 and lib.dvmvs_abi_version() == 11

"""Generates the fixtures of the DPSNet baseline by RUNNING THE REFERENCE on CPU in the build container.

    python tests/golden/make_dpsnet_goldens.py

Writes (see reference_import.py for how the reference is imported; nothing of it is copied; inputs: tests/dpsnet_fixtures.py):
  dpsnet_state_dict_keys.json  parameter / buffer names and shapes of the reference's PSNet(64, 0.5)
  dpsnet_bn_stats.npz          BatchNorm statistics of the seeded module, calibrated on the first frame
  dpsnet_volume.npz            inverse_warp plane volumes (the warped half; the other half is the reference features): five sample-scene
                               pose pairs at 60x80, C = 32, 64 planes as pins (fp32 and float64 evaluations at the pinned elements), two
                               small ragged cases in full; with each case its pose, K, K^-1, the flat [B,nlabel,h,w] indices of the
                               pixels whose un-masked coordinate lies within 1e-4 of +-1, and max|fp32 - float64| over the rest
  dpsnet_regress.npz           up-sampling + softmax + expectation on random and adversarial cost volumes, from the reference
                               expressions in fp32 and float64, with the fp32 chain's own error against float64
  dpsnet_e2e.npz               three lines of the sample scene's nmeas+2 index and one "TRACKING LOST" at 320x240, and one frame at
                               128x160: pins of the quarter-resolution features, costs, costss, pred0, pred, depth0, depth; the
                               factors of the last classify / convs layers (dpsnet_fixtures.scale_last_layers)
"""
import importlib
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import dpsnet_fixtures as fx  # noqa: E402
import synthetic as syn  # noqa: E402
from reference_import import REFERENCE_ROOT, import_reference  # noqa: E402

torch.set_num_threads(8)
NEAR_MASK = 1e-4


def save(name, arrays):
    out = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrays.items()}
    np.savez_compressed(os.path.join(HERE, name), **out)
    print(f"wrote {name}: {os.path.getsize(os.path.join(HERE, name + '.npz')) / 1024:.0f} KiB")


def pins(prefix, t):
    p = syn.tensor_pins(t)
    return {f"{prefix}_shape": p["shape"], f"{prefix}_sum": p["sum"], f"{prefix}_abs_sum": p["abs_sum"], f"{prefix}_samples": p["samples"]}


# ---- plane volumes --------------------------------------------------------------------------------------------------------------------
def reference_volume(dps, meas, pose, K4, Kinv4, nlabel):
    """(warped [B,C,nlabel,h,w], un-masked coordinates [B,nlabel,h,w,2]) from the reference's inverse_warp / cam2pixel, in meas.dtype."""
    b, c, h, w = meas.shape
    dps.pixel_coords = None              # the reference caches its pixel grid in a module global, in the dtype of its first call
    disp2depth = torch.ones((b, h, w), dtype=meas.dtype) * fx.MINDEPTH * nlabel
    warped = torch.zeros((b, c, nlabel, h, w), dtype=meas.dtype)
    coords = torch.zeros((b, nlabel, h, w, 2), dtype=meas.dtype)
    for i in range(nlabel):
        depth = torch.div(disp2depth, i + 1e-16)
        warped[:, :, i] = dps.inverse_warp(meas, depth, pose, K4, Kinv4)
        proj = K4.bmm(pose)
        coords[:, i] = dps.cam2pixel(dps.pixel2cam(depth, Kinv4), proj[:, :, :3], proj[:, :, -1:], "border")
    return warped, coords


def volume_case(dps, arrays, tag, meas, pose, K4, Kinv4, nlabel, full):
    w32, coords = reference_volume(dps, meas, pose, K4, Kinv4, nlabel)
    w64, _ = reference_volume(dps, meas.double(), pose.double(), K4.double(), Kinv4.double(), nlabel)
    near = ((coords.abs() - 1).abs() < NEAR_MASK).any(dim=-1)                       # [B,nlabel,h,w]
    masked = ((coords.abs() > 1).any(dim=-1)).float().mean().item()
    keep = ~near.unsqueeze(1).expand(-1, meas.shape[1], -1, -1, -1)
    err = ((w32.double() - w64).abs() * keep).max().item()
    arrays.update({f"{tag}_pose": pose, f"{tag}_K4": K4, f"{tag}_Kinv4": Kinv4, f"{tag}_near": torch.nonzero(near.reshape(-1)).reshape(-1),
                   f"{tag}_ref_err": err})
    if full:
        arrays.update({f"{tag}_warped": w32, f"{tag}_warped64": w64})
    else:
        idx = syn.sample_indices(w32.numel(), fx.VOLUME_PIN_COUNT)
        arrays.update({f"{tag}_samples": w32.reshape(-1)[idx], f"{tag}_samples64": w64.reshape(-1)[idx], f"{tag}_sum": w32.double().sum().item(),
                       f"{tag}_abs_sum": w32.double().abs().sum().item()})
    print(f"volume {tag}: masked {masked:.3f}, near the mask {near.float().mean().item():.2e}, max|fp32 - f64| {err:.3e}")


def volume_goldens(dps):
    arrays = {}
    K4, Kinv4 = fx.quarter(*fx.intrinsics(320, 240))
    for n, (r, m) in enumerate(fx.VOLUME_PAIRS):
        _, meas = fx.feature_maps(1, 32, 60, 80, seed=300 + 2 * n)
        volume_case(dps, arrays, f"pair{n}", meas, fx.relative_pose(r, m), K4, Kinv4, fx.NLABEL, full=False)
    for n, (tag, B, C, nlabel, h, w, pairs) in enumerate(fx.VOLUME_SMALL):
        _, meas = fx.feature_maps(B, C, h, w, seed=400 + 2 * n)
        Ks, Ksinv = fx.small_intrinsics(B, h, w)
        volume_case(dps, arrays, tag, meas, torch.cat([fx.relative_pose(r, m) for r, m in pairs], 0), Ks, Ksinv, nlabel, full=True)
    save("dpsnet_volume", arrays)


# ---- regression ----------------------------------------------------------------------------------------------------------------------
def reference_regress(dps, costs, nlabel, H, W):
    """(pred [B,H,W], depth [B,1,H,W]) with the expressions of dpsnet.py:373-383 in costs.dtype."""
    up = torch.squeeze(F.interpolate(costs, [nlabel, H, W], mode="trilinear", align_corners=False), 1)
    pred = dps.disparityregression(nlabel)(F.softmax(up, dim=1))
    return pred, fx.MINDEPTH * nlabel / (pred.unsqueeze(1) + 1e-16)


def regress_goldens(dps):
    arrays = {}
    for s, (size, nlabel, h, w, H, W) in enumerate(fx.REGRESS_SIZES):
        for k, kind in enumerate(fx.REGRESS_KINDS):
            tag = f"{size}_{kind}"
            costs = fx.regress_costs(kind, nlabel, h, w, seed=500 + 10 * s + k)
            p32, d32 = reference_regress(dps, costs, nlabel, H, W)
            p64, d64 = reference_regress(dps, costs.double(), nlabel, H, W)
            ok = p64 >= 0.5
            arrays[f"{tag}_pred_err"] = (p32.double() - p64).abs().max().item()
            arrays[f"{tag}_depth_rel_err"] = ((d32.double() - d64).abs() / d64)[ok.unsqueeze(1)].max().item() if ok.any() else 0.0
            if size == "full":
                idx = syn.sample_indices(p32.numel(), fx.REGRESS_PIN_COUNT)
                for name, t in (("pred", p32), ("pred64", p64), ("depth", d32), ("depth64", d64)):
                    arrays[f"{tag}_{name}_samples"] = t.reshape(-1)[idx]
            else:
                arrays.update({f"{tag}_pred": p32, f"{tag}_pred64": p64, f"{tag}_depth": d32, f"{tag}_depth64": d64})
            print(f"regress {tag}: pred mean {p64.mean().item():.3f}, fp32 error {arrays[f'{tag}_pred_err']:.3e}, depth rel "
                  f"{arrays[f'{tag}_depth_rel_err']:.3e}, finite {bool(torch.isfinite(d32).all())}")
    save("dpsnet_regress", arrays)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
class Recorder:
    """Forward hooks on the reference module: the quarter-resolution reference features (first feature_extraction call), the plane
    costs of every measurement frame (classify) and the per-plane outputs of the context network (convs)."""

    def __init__(self, net):
        self.features, self.classify, self.convs = [], [], []
        net.feature_extraction.register_forward_hook(lambda m, i, o: self.features.append(o.detach().clone()))
        net.classify.register_forward_hook(lambda m, i, o: self.classify.append(o.detach().clone()))
        net.convs.register_forward_hook(lambda m, i, o: self.convs.append(o.detach().clone()))

    def clear(self):
        self.features, self.classify, self.convs = [], [], []


def run_frame(dps, net, rec, line, height, width):
    """One frame in the order of dpsnet/run-testing.py:79-126; returns the pinned tensors."""
    r, ms = line
    K, Kinv = fx.intrinsics(width, height)
    rec.clear()
    dps.pixel_coords = None
    with torch.no_grad():
        depth0, depth = net(fx.e2e_image(r, height, width), [fx.e2e_image(m, height, width) for m in ms], [fx.relative_pose(r, m) for m in ms],
                            K, Kinv)
    costs = sum(rec.classify) / len(ms)
    convs_out = torch.stack(rec.convs, 2)                        # [B,1,nlabel,h,w]
    costss = convs_out + costs
    pred0, d0 = reference_regress(dps, costs, fx.NLABEL, height, width)
    pred, d1 = reference_regress(dps, costss, fx.NLABEL, height, width)
    assert torch.equal(d0, depth0) and torch.equal(d1, depth), "the recorded intermediates do not reproduce the reference's outputs"
    return {"features": rec.features[0], "costs": costs, "costss": costss, "convs_out": convs_out, "pred0": pred0, "pred": pred,
            "depth0": depth0, "depth": depth}


def well_conditioned(out):
    """The issue's condition on a pinned frame: fewer than 5 % of the pixels with pred < 0.5, at least 16 distinct arg-max planes."""
    ok = True
    for key, vol in (("pred0", "costs"), ("pred", "costss")):
        low = (out[key] < 0.5).float().mean().item()
        distinct = F.interpolate(out[vol], [fx.NLABEL, *out[key].shape[1:]], mode="trilinear", align_corners=False).argmax(2).unique().numel()
        print(f"    {key}: {100 * low:.2f} % below 0.5, {distinct} distinct arg-max planes, mean {out[key].mean().item():.2f}")
        ok = ok and low < 0.05 and distinct >= 16
    return ok


def e2e_goldens(dps):
    net = fx.seed_weights(dps.PSNet(fx.NLABEL, fx.MINDEPTH))
    net.eval()
    with open(os.path.join(HERE, "dpsnet_state_dict_keys.json"), "w") as f:
        json.dump({k: list(v.shape) for k, v in net.state_dict().items()}, f, indent=0)
    rec = Recorder(net)
    lines = syn.keyframe_index_lines(2)
    H, W = 240, 320

    # BatchNorm statistics = the batch statistics of one forward pass of the first frame (2-d and 3-d layers)
    bns = [m for m in net.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
    for m in bns:
        m.momentum = 1.0
        m.train()
    run_frame(dps, net, rec, lines[0], H, W)
    for m in bns:
        m.momentum = 0.1
        m.eval()
    save("dpsnet_bn_stats", syn.collect_bn_stats([("dpsnet", net)]))

    # factors of the two last layers: spread of the costs over the planes ~ 3, of the context network's residual ~ 1
    out = run_frame(dps, net, rec, lines[0], H, W)
    f1 = float(f"{3.0 / out['costs'].std(dim=2).mean().item():.3g}")
    fx.scale_last_layers(net, f1, 1.0)
    out = run_frame(dps, net, rec, lines[0], H, W)
    f2 = float(f"{1.0 / out['convs_out'].std(dim=2).mean().item():.3g}")
    fx.scale_last_layers(net, 1.0, f2)
    schedule = [e for e in fx.E2E_SCHEDULE if e is not None]
    for attempt in range(8):
        print(f"factors: classify {f1}, convs {f2}")
        frames = [run_frame(dps, net, rec, lines[e], H, W) for e in schedule]
        small = run_frame(dps, net, rec, lines[0], *fx.E2E_SMALL)
        if all([well_conditioned(o) for o in frames + [small]]):
            break
        fx.scale_last_layers(net, 0.5, 0.5)
        f1, f2 = f1 * 0.5, f2 * 0.5
    else:
        raise RuntimeError("no factors found that keep the soft-argmin off plane 0")

    arrays = {"factors": np.array([f1, f2]), "schedule": np.array([-1 if e is None else e for e in fx.E2E_SCHEDULE]), "n_frames": len(frames)}
    for tag, line, o, (h, w) in [(f"f{n}", lines[e], frames[n], (H, W)) for n, e in enumerate(schedule)] + [("small", lines[0], small, fx.E2E_SMALL)]:
        r, ms = line
        K, Kinv = fx.intrinsics(w, h)
        arrays.update({f"{tag}_frames": np.array([r, *ms]), f"{tag}_K": K, f"{tag}_Kinv": Kinv,
                       f"{tag}_poses": torch.cat([fx.relative_pose(r, m) for m in ms], 0)})
        for key in ("features", "costs", "costss", "pred0", "pred", "depth0", "depth"):
            arrays.update(pins(f"{tag}_{key}", o[key]))
    save("dpsnet_e2e", arrays)


def main():
    import_reference()
    dps = importlib.import_module("dvmvs.baselines.dpsnet.dpsnet")
    assert dps.__file__.startswith(REFERENCE_ROOT)
    volume_goldens(dps)
    regress_goldens(dps)
    e2e_goldens(dps)


if __name__ == "__main__":
    main()

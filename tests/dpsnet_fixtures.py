"""Inputs shared by tests/golden/make_dpsnet_goldens.py (which runs the reference) and the DPSNet tests: everything a test has to
rebuild on its own machine to meet the fixtures -- seeded weights, feature maps, poses, cost volumes.  Imports nothing of the
``dvmvs`` package (the generator process holds the reference's package of that name)."""
import os
import zlib

import numpy as np
import torch

import synthetic as syn

NLABEL, MINDEPTH = 64, 0.5
MODULE_SEED = 20
# sample-scene pose pairs (reference, measurement) of the pinned plane volumes; the fourth has 74 % of its samples masked, the fifth 40 %
VOLUME_PAIRS = ((9, 6), (9, 0), (12, 10), (141, 135), (200, 195))
VOLUME_PIN_COUNT = 8192
# (tag, B, C, nlabel, h, w, pose pairs per batch item): small ragged cases kept in full
VOLUME_SMALL = (("small_a", 1, 5, 13, 19, 27, ((9, 6),)), ("small_b", 2, 3, 7, 11, 14, ((12, 10), (9, 0))))
# lines of the sample scene's nmeas+2 index (synthetic.keyframe_index_lines), None = "TRACKING LOST"
E2E_SCHEDULE = (0, 1, None, 2)
E2E_SMALL = (128, 160)        # one more frame (line 0) at this size: the CPU test's
REGRESS_KINDS = ("random", "peak", "equal", "big")
# (tag, nlabel, h, w, H, W): the first as pins, the others in full (the last with non-integer up-sampling ratios)
REGRESS_SIZES = (("full", 64, 60, 80, 240, 320), ("x4", 64, 7, 9, 28, 36), ("ragged", 13, 5, 6, 17, 23))
REGRESS_PIN_COUNT = 8192


def golden(name):
    return np.load(os.path.join(syn.GOLDEN_DIR, name))


# ---- poses and intrinsics ------------------------------------------------------------------------------------------------------------
def relative_pose(reference_index, measurement_index):
    """[1,3,4] float32: (inv(measurement) @ reference)[0:3] in float64, then cast (dpsnet/run-testing.py:110-112)."""
    poses = syn.sample_poses()
    return torch.from_numpy((np.linalg.inv(poses[measurement_index]) @ poses[reference_index])[0:3, :]).float().unsqueeze(0)


def intrinsics(width, height):
    """(K, K^-1) [1,3,3] float32 of the sample scene at this input size; the inverse by np.linalg.inv as run-testing.py takes it."""
    K = syn.full_K(width, height)
    return K, torch.from_numpy(np.linalg.inv(K[0].numpy().astype(np.float64))).float().unsqueeze(0)


def quarter(K, Kinv):
    """PSNet.forward's quarter-resolution intrinsics (dpsnet.py:335-338)."""
    K4, Kinv4 = K.clone(), Kinv.clone()
    K4[:, :2, :] = K4[:, :2, :] / 4
    Kinv4[:, :2, :2] = Kinv4[:, :2, :2] * 4
    return K4, Kinv4


def small_intrinsics(B, h, w):
    K = torch.tensor([[[0.9 * w, 0.0, w / 2.0], [0.0, 0.9 * w, h / 2.0], [0.0, 0.0, 1.0]]])
    Kinv = torch.from_numpy(np.linalg.inv(K[0].numpy().astype(np.float64))).float().unsqueeze(0)
    return K.expand(B, 3, 3).contiguous(), Kinv.expand(B, 3, 3).contiguous()


def feature_maps(B, C, h, w, seed):
    """(reference, measurement) feature maps: smooth noise with texture at the scale of a few pixels."""
    return syn.smooth_noise((B, C, h, w), seed=seed, passes=1), syn.smooth_noise((B, C, h, w), seed=seed + 1, passes=1)


def e2e_image(index, height, width):
    return syn.e2e_image(index)[:, :, :height, :width].contiguous()


# ---- cost volumes of the regression tests -----------------------------------------------------------------------------------------
def regress_costs(kind, nlabel, h, w, seed):
    """[1,1,nlabel,h,w] plane costs: 'random' N(0, 3^2); 'peak' N(0,1) with one plane per pixel 30 above the rest; 'equal' every plane
    of a pixel the same value; 'big' values around +-80 (a softmax without max-subtraction overflows)."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn((1, 1, nlabel, h, w), generator=g)
    if kind == "random":
        return base * 3.0
    if kind == "peak":
        k = torch.randint(0, nlabel, (1, 1, 1, h, w), generator=g)
        return base.scatter_add(2, k, torch.full((1, 1, 1, h, w), 30.0))
    if kind == "equal":
        return base[:, :, :1].expand(1, 1, nlabel, h, w).contiguous()
    if kind == "big":
        sign = torch.where(torch.rand((1, 1, nlabel, h, w), generator=g) < 0.5, -1.0, 1.0)
        return sign * 80.0 + base
    raise ValueError(kind)


# ---- the seeded module ---------------------------------------------------------------------------------------------------------------
def seed_weights(module):
    """Deterministic weights keyed on the state-dict names (synthetic.deterministic_init; the 5-d weights of the 3-D convolutions,
    which that function would treat as BatchNorm weights, get N(0, 2 / fan_in) like the 2-d ones)."""
    syn.deterministic_init(module, seed=MODULE_SEED)
    with torch.no_grad():
        for name, t in sorted(module.state_dict().items()):
            if t.dim() == 5:
                g = torch.Generator().manual_seed((zlib.crc32(name.encode()) + 7919 * MODULE_SEED) % (2 ** 31))
                fan_in = t.shape[1] * t.shape[2] * t.shape[3] * t.shape[4]
                t.copy_(torch.randn(t.shape, generator=g) * (2.0 / fan_in) ** 0.5)
    return module


def scale_last_layers(module, classify_factor, convs_factor):
    """The generator's conditioning of the seeded module: the last ``classify`` convolution and the last ``convs`` layer are scaled so
    that the soft-argmin does not saturate (make_dpsnet_goldens.py records the factors in dpsnet_e2e.npz)."""
    with torch.no_grad():
        module.classify[-1].weight.mul_(float(classify_factor))
        module.convs[-1][0].weight.mul_(float(convs_factor))
    return module


def seeded_dpsnet(ctor):
    """``ctor(NLABEL, MINDEPTH)`` with the weights, BatchNorm statistics and factors of the fixtures, in eval mode."""
    module = seed_weights(ctor(NLABEL, MINDEPTH))
    syn.apply_bn_stats([("dpsnet", module)], os.path.join(syn.GOLDEN_DIR, "dpsnet_bn_stats.npz"))
    factors = golden("dpsnet_e2e.npz")["factors"]
    scale_last_layers(module, factors[0], factors[1])
    module.eval()
    return module


def rel_l1(got, pins):
    idx = syn.sample_indices(got.numel())
    g = got.reshape(-1)[idx].double().cpu()
    w = torch.from_numpy(np.asarray(pins)).double()
    return ((g - w).abs().sum() / w.abs().sum()).item()

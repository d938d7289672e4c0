"""The frame sizes at which DepthEngine is tested besides its 320x256 (tests/test_engine_sizes_host.py on the CPU, tests/test_engine_sizes_gpu.py
on the GPU), the inputs of those runs, how their fixtures (tests/golden/engine_sizes_<W>x<H>.npz and ..._state.npz, written by
tests/golden/make_engine_size_goldens.py) store state and results, the criterion, and the kernel problems each size sends to the HIP convolution
kernels at batch 1.  A plain helper module: no GPU and no library needed to import it.

Two fixture files per size, the installed state and the results: a committed file stays under 1 MiB.  That is also why
* the recurrent state that is installed before frames 2 and 3 (teacher forcing) is the float32 CPU pipeline's state ROUNDED to a short format
  -- h and c to one byte each, multiples of a power-of-two step that the tensor's range sets (1/64 ... 1/16 here: no value is clipped), the
  previous depth to float16 -- and every evaluation (float32 CPU, float64 CPU, the engine) starts the frame from those rounded values, which
  all three hold exactly;
* results are kept as what the criterion reads.  h / c / bottom / cost volume / features: ``syn.sample_indices`` samples, plus the whole tensor's
  sum and sum of magnitudes.  The depth: the whole map on the two small frames; on the larger ones DEPTH_SAMPLES pixels drawn uniformly (every
  residue of every tile, an unbiased estimate of the whole map's rel-L1), the whole two-pixel border of the map (first / last two rows and
  columns: where a 5x5 layer's padding, a tile's tail and a ragged last row tile show), and at every size the mean of every 8x8 block of the
  map and the map's sum, to which every pixel contributes.
"""
import os

import numpy as np
import torch

import synthetic as syn

SIZES = [(96, 64), (160, 128), (256, 256), (320, 256), (640, 512)]      # (W, H)
REFUSED_SIZES = [(330, 256), (320, 240), (0, 256)]                       # no multiple of 32: DepthEngine.__init__ raises ValueError
SLACK = 3.0                                                               # tests/accuracy.as_accurate_as_reference's constant
DEPTH_STAGES = ("depth", "depth_border", "depth_blocks")                 # rel-L1 on the drawn pixels (or the whole map), on the border, of the block means
CRITERION_STAGES = DEPTH_STAGES + ("h", "c", "bottom", "cost_volume")    # what must meet the criterion; "feat_half" is reported with them
STAGES = CRITERION_STAGES + ("feat_half",)
SAMPLED = ("h", "c", "bottom", "cost_volume", "feat_half")
DEPTH_SAMPLES = 49152


def size_id(size):
    return f"{size[0]}x{size[1]}"


def frames(W, H):
    """(reference pose index, measurement pose indices) per frame: the three golden frames, the first two at the largest size (its float64
    evaluation takes 15 s per frame)."""
    return list(syn.E2E_FRAMES[:2] if (W, H) == (640, 512) else syn.E2E_FRAMES)


def image(index, W, H):
    """``syn.e2e_image`` with a size."""
    return syn.smooth_noise((1, 3, H, W), seed=2000 + index)


def full_K(W, H):
    return syn.full_K(W, H)


def fixture_path(W, H, golden_dir=syn.GOLDEN_DIR):
    return os.path.join(golden_dir, f"engine_sizes_{W}x{H}.npz")


def state_path(W, H, golden_dir=syn.GOLDEN_DIR):
    return os.path.join(golden_dir, f"engine_sizes_{W}x{H}_state.npz")


def is_state(name):
    """Whether an array of a size's fixture belongs into its state file."""
    return "_state_" in name


def load_fixture(W, H, golden_dir=syn.GOLDEN_DIR):
    """The size's two files as one dict."""
    return {**np.load(fixture_path(W, H, golden_dir)), **np.load(state_path(W, H, golden_dir))}


# ---- the installed state ----------------------------------------------------------------------------------------------------------------
def _to_bytes(t):
    """(int8 array, step): ``t`` rounded to multiples of the smallest power of two ``step`` >= 1/64 for which every value fits one byte -- the
    range follows the tensor, so the installed state is the network's own, rounded, never clipped."""
    step = 1.0 / 64.0
    while float(t.abs().max()) > 127.0 * step:
        step *= 2.0
    return torch.round(t.float() / step).to(torch.int8).numpy(), np.float32(step)


def pack_state(h, c, depth):
    """(h, c, previous depth) of the float32 pipeline -> the short arrays the fixture stores."""
    (hq, h_step), (cq, c_step) = _to_bytes(h), _to_bytes(c)
    return {"h_q": hq, "h_step": h_step, "c_q": cq, "c_step": c_step, "depth_q": depth.float().to(torch.float16).numpy()}


def unpack_state(z, prefix):
    """The installed state as float32 tensors: exactly the values every evaluation of the frame started from."""
    h = torch.from_numpy(z[f"{prefix}_h_q"].astype(np.float32)) * float(z[f"{prefix}_h_step"])
    c = torch.from_numpy(z[f"{prefix}_c_q"].astype(np.float32)) * float(z[f"{prefix}_c_step"])
    depth = torch.from_numpy(z[f"{prefix}_depth_q"].astype(np.float32))
    return h, c, depth


# ---- what is stored of a result, and the distances -----------------------------------------------------------------------------------------
def depth_pixels(W, H):
    """(flat indices of the pixels "depth" is read on, of the two-pixel border): the whole map on the small frames, else DEPTH_SAMPLES pixels drawn
    uniformly with a fixed seed."""
    rows, cols = np.arange(H).reshape(-1, 1), np.arange(W).reshape(1, -1)
    on_border = (rows < 2) | (rows >= H - 2) | (cols < 2) | (cols >= W - 2)
    border = np.flatnonzero(on_border)
    if W * H <= 160 * 128:
        return np.arange(W * H), border
    return syn.sample_indices(W * H, count=DEPTH_SAMPLES, seed=4321).numpy(), border


def depth_values(depth, W, H):
    """{"depth", "depth_border": float64 values on depth_pixels, "depth_blocks": the mean of every 8x8 block, "sum": the map's sum} of a depth map
    given as tensor or array of H * W elements."""
    d = depth.detach().cpu().double().numpy() if isinstance(depth, torch.Tensor) else np.asarray(depth, dtype=np.float64)
    d = d.reshape(H, W)
    drawn, border = depth_pixels(W, H)
    return {"depth": d.reshape(-1)[drawn], "depth_border": d.reshape(-1)[border],
            "depth_blocks": d.reshape(H // 8, 8, W // 8, 8).mean(axis=(1, 3)).reshape(-1), "sum": float(d.sum())}


def samples(t):
    """The ``syn.sample_indices`` entries of a tensor, float64 numpy."""
    flat = t.detach().reshape(-1)
    return flat[syn.sample_indices(flat.numel()).to(flat.device)].cpu().double().numpy()


def depth_distance(d, d64):
    """rel-L1, mean(|d - d64| / d64)."""
    return float(np.mean(np.abs(d - d64) / d64))


def distance(x, x64):
    """mean |x - x64| / mean |x64|."""
    return float(np.mean(np.abs(x - x64)) / np.mean(np.abs(x64)))


def flipped_pixels(a, b):
    """Pixels of the low-resolution depth estimate that two evaluations took from different source points (tests/test_e2e_gpu.py's count)."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    return int(np.sum(np.abs(a - b) > 1e-3 * np.maximum(np.maximum(a, b), 1e-3)))


def yardsticks(z, W, H):
    """{stage: the float32 CPU pipeline's own distance from the float64 one, the largest over the size's frames} out of the fixture ``z``."""
    return {stage: max(float(z[f"f{n}_{stage}_yardstick"]) for n in range(len(frames(W, H)))) for stage in STAGES}


def result_distances(z, n, W, H, depth, **tensors):
    """{stage: distance of a result of frame ``n`` from the fixture's float64 values}; ``tensors``: h, c, bottom, cost_volume, feat_half."""
    values = depth_values(depth, W, H)
    out = {stage: depth_distance(values[stage], z[f"f{n}_{stage}64"].astype(np.float64)) for stage in DEPTH_STAGES}
    for stage in SAMPLED:
        out[stage] = distance(samples(tensors[stage]), z[f"f{n}_{stage}64_samples"].astype(np.float64))
    return out


def sum_distances(z, n, W, H, depth, **tensors):
    """{stage: (|sum - sum64| / abs_sum64, |abs_sum - abs_sum64| / abs_sum64)} of the WHOLE tensors of frame ``n``.  Both are at most the tensor's
    mean |x - x64| / mean |x64| (triangle inequality), the quantity the stage's yardstick measures on the samples: SLACK times the yardstick bounds
    them where the criterion holds on the whole tensor, and a region the samples miss that is wrong by its own magnitude breaks it."""
    out = {"depth": (abs(float(depth.double().sum()) - float(z[f"f{n}_depth64_sum"])) / float(z[f"f{n}_depth64_sum"]), 0.0)}
    for stage in SAMPLED:
        t, total = tensors[stage].double(), float(z[f"f{n}_{stage}64_abs_sum"])
        out[stage] = (abs(float(t.sum()) - float(z[f"f{n}_{stage}64_sum"])) / total, abs(float(t.abs().sum()) - total) / total)
    return out


# ---- the kernel problems of a size at batch 1 ----------------------------------------------------------------------------------------------
# What the engine's fused, BN-folded, destination-passing frame body sends where, over the size's frames (the measurement frames' features of the
# first frame included: they take FeatureShrinker.forward, which also computes the FPN's 1/32 output): recorded on the GPU by
# tests/test_engine_sizes_gpu.py::test_dispatch, derived on the CPU from the layers and the library's shape rules by tests/test_engine_sizes_host.py.
#   bottleneck: (C_in, C_out, H, W, stride) -- tests/test_bottleneck_conv_gpu.py::SHAPES's form; H, W of the map the layer convolves
#   up2x:       the bottleneck problems whose input is up-sampled in the kernel's staging (forward_upsampled)
#   lstm:       "bottleneck" or "library": where the ConvLSTM's 1024 -> 2048 convolution runs
#   direct:     (C_in, H, W, C_out, k, stride) -- tests/test_direct_conv_host.py::FRAME_LAYERS's form
#   head:       (C_in, H, W) of the one-channel 3x3 depth heads
#   pointwise:  (C_in, C_out, H, W) -- tests/test_pointwise_conv_gpu.py::FRAME_SHAPES's form
#   library:    (C_in, C_out, H, W, k, stride) of the dense convolutions left to the library
#   sweep:      the plane sweep's variants the frames may run (which of the tiled ones a geometry gets is the host plan's choice)
#
# The network's layers do not depend on the size, only their maps do: a layer is written with the divisor of the frame its INPUT map has.
DENSE_LAYERS = [  # (C_in, C_out, divisor, k, stride): every dense 3x3 / 5x5 layer with more than one output channel, once per distinct problem
    (3, 32, 1, 3, 2),                                                                                      # MnasNet's stem
    (32, 32, 2, 3, 1), (32, 32, 4, 3, 1), (32, 32, 8, 3, 1), (32, 32, 16, 3, 1), (32, 32, 32, 3, 1),        # the FPN's output layers (1/32: measurement frames only)
    # encoder levels 0 .. 3: aggregator, stride-2 down-convolution, the block's standard layers
    (96, 32, 2, 5, 1), (32, 64, 2, 5, 2), (64, 64, 4, 5, 1),
    (96, 64, 4, 3, 1), (64, 128, 4, 3, 2), (128, 128, 8, 3, 1),
    (160, 128, 8, 3, 1), (128, 256, 8, 3, 2), (256, 256, 16, 3, 1),
    (288, 256, 16, 3, 1), (256, 512, 16, 3, 2), (512, 512, 32, 3, 1),
    # decoder blocks 1 .. 4: up-convolution on the up-sampled map, [up | skip | depth] -> block, block's second layer (block 1's second layer is
    # encoder level 2's (256, 256, 16), block 2's encoder level 1's (128, 128, 8)); the refinement layers
    (512, 256, 16, 3, 1),
    (256, 128, 8, 3, 1), (257, 128, 8, 3, 1),
    (128, 64, 4, 3, 1), (129, 64, 4, 3, 1), (64, 64, 4, 3, 1),
    (64, 32, 2, 5, 1), (65, 32, 2, 5, 1), (32, 32, 2, 5, 1),
    (36, 32, 1, 5, 1), (32, 32, 1, 5, 1),
]
POINTWISE_LAYERS = [  # (C_in, C_out, divisor): MnasNet's expansion / projection layers, then the FPN's lateral layers (the last four add the coarser level)
    (32, 16, 2), (16, 48, 2), (48, 24, 4), (24, 72, 4), (72, 24, 4), (72, 40, 8), (40, 120, 8), (120, 40, 8), (40, 240, 8), (240, 80, 16), (80, 480, 16),
    (480, 80, 16), (480, 96, 16), (96, 576, 16), (576, 96, 16), (576, 192, 32), (192, 1152, 32), (1152, 192, 32), (1152, 320, 32), (320, 32, 32),
    (96, 32, 16), (40, 32, 8), (24, 32, 4), (16, 32, 2),
]
POINTWISE_ADDS_COARSER = POINTWISE_LAYERS[-4:]      # their epilogue adds the nearest-up-sampled coarser level (residual mode 2: needs W % 4 == 0)
HEAD_LAYERS = [(256, 16), (128, 8), (64, 4), (32, 2), (32, 1)]      # (C_in, divisor) of the decoder's depth heads


def dense_problems(W, H):
    """DENSE_LAYERS at a size, in the library form (C_in, C_out, H, W, k, stride)."""
    return sorted((ci, co, H // d, W // d, k, s) for ci, co, d, k, s in DENSE_LAYERS)


def pointwise_problems(W, H):
    return sorted((ci, co, H // d, W // d) for ci, co, d in POINTWISE_LAYERS)


def lateral_problems(W, H):
    """(C_in, C_out, H, W) of the lateral layers that add the up-sampled coarser level, where the pointwise kernel takes them."""
    return sorted((ci, co, H // d, W // d) for ci, co, d in POINTWISE_ADDS_COARSER if (ci, co, H // d, W // d) in EXPECTED[(W, H)]["pointwise"])


def _expected(W, H, bottleneck, library_dense, library_pointwise, lstm, sweep, up2x=()):
    """A size's entry: what is not named goes to the direct kernel (dense layers) or to the pointwise kernel (1x1 layers)."""
    dense, taken = dense_problems(W, H), {(ci, co, h, w, 3, s) for ci, co, h, w, s in bottleneck}
    assert taken <= set(dense) and set(library_dense) <= set(dense) - taken and set(library_pointwise) <= set(pointwise_problems(W, H))
    return {"bottleneck": sorted(bottleneck), "up2x": sorted(up2x), "lstm": [lstm],
            "direct": sorted((ci, h, w, co, k, s) for ci, co, h, w, k, s in set(dense) - taken - set(library_dense)),
            "head": sorted((ci, H // d, W // d) for ci, d in HEAD_LAYERS),
            "pointwise": sorted(set(pointwise_problems(W, H)) - set(library_pointwise)),
            "library": sorted(list(library_dense) + [(ci, co, h, w, 1, 1) for ci, co, h, w in library_pointwise]), "sweep": list(sweep)}


EXPECTED = {
    # no output width is a multiple of 40: every dense layer is the library's; the 1x1 layers of the 2x3 map (H * W % 4) and the lateral layer that
    # adds it (W % 4 of the 4x6 map) too; 32x48 cells are fewer than the MFMA sweep takes: the tiled sweep from its work list
    (96, 64): _expected(96, 64, [], dense_problems(96, 64),
                        [(576, 192, 2, 3), (192, 1152, 2, 3), (1152, 192, 2, 3), (1152, 320, 2, 3), (320, 32, 2, 3), (96, 32, 4, 6)], "library", [2, 3, 4, 5]),
    # the bottleneck kernel takes the 1/16 (8x10), 1/8 (16x20) layers and the stride-2 layer of the 1/4 (32x40) map
    (160, 128): _expected(160, 128, [(32, 32, 8, 10, 1), (32, 32, 16, 20, 1), (64, 128, 32, 40, 2), (128, 128, 16, 20, 1), (128, 256, 16, 20, 2),
                                     (160, 128, 16, 20, 1), (256, 128, 16, 20, 1), (256, 256, 8, 10, 1), (288, 256, 8, 10, 1), (512, 256, 8, 10, 1)],
                          [(32, 32, 4, 5, 3, 1), (256, 512, 8, 10, 3, 2), (257, 128, 16, 20, 3, 1), (512, 512, 4, 5, 3, 1)], [(96, 32, 8, 10)], "library", [6]),
    (256, 256): _expected(256, 256, [], dense_problems(256, 256), [], "library", [6]),
    (320, 256): _expected(320, 256, [(32, 32, 8, 10, 1), (32, 32, 16, 20, 1), (128, 256, 32, 40, 2), (256, 256, 16, 20, 1), (256, 512, 16, 20, 2),
                                     (288, 256, 16, 20, 1), (512, 256, 16, 20, 1), (512, 512, 8, 10, 1)], [], [], "bottleneck", [6],
                          up2x=[(512, 256, 16, 20, 1)]),
    (640, 512): _expected(640, 512, [(32, 32, 16, 20, 1), (256, 512, 32, 40, 2), (512, 512, 16, 20, 1)], [], [], "bottleneck", [6]),
}
LSTM_PROBLEM = (1024, 2048)      # (C_in, C_out) of the ConvLSTM's 3x3 convolution on the 1/32 map

"""CPU checks behind tests/test_engine_sizes_gpu.py (no GPU: the kernels' shape rules are host functions of libdvmvs_hip.so):
* the layer tables of tests/engine_size_cases.py are the network's layers (its modules run on shape-only tensors at every size);
* sent through the shape rules in FusedConv2d's order they give each size's expected problem lists;
* the problems of those lists have kernel-level pins: the bottleneck problems are in test_bottleneck_conv_gpu.SHAPES, the direct problems run a
  kernel that tests/direct_conv_cases.py pins, the pointwise test takes its size shapes from the lists, the conv-head shapes hold the two the
  issue names and every head's channel count and kernel form;
* the generator reproduces the smallest fixture on this CPU."""
import importlib.util
import os

import numpy as np
import pytest
import torch
from torch import nn

import direct_conv_cases as dc
import engine_size_cases as cases
from dvmvs.hip import _capi


def lib():
    return _capi.lib()


# ---- the layer tables are the network ------------------------------------------------------------------------------------------------------
def traced_layers(W, H):
    """{(C_in, C_out, H, W, k, stride, groups)} of every convolution the five modules run on a W x H frame, the ConvLSTM's included: the modules
    themselves, on tensors that have a shape and no storage."""
    from dvmvs.fusionnet.model import CostVolumeDecoder, CostVolumeEncoder, FeatureExtractor, FeatureShrinker, LSTMFusion
    seen = set()

    def record(module, inputs, output):
        x = inputs[0]
        seen.add((x.shape[1], module.out_channels, x.shape[2], x.shape[3], module.kernel_size[0], module.stride[0], module.groups))

    with torch.device("meta"):
        fe, fs, enc, lstm, dec = (ctor().eval() for ctor in (FeatureExtractor, FeatureShrinker, CostVolumeEncoder, LSTMFusion, CostVolumeDecoder))
    for m in (fe, fs, enc, lstm, dec):
        for sub in m.modules():
            if isinstance(sub, nn.Conv2d):
                sub.register_forward_hook(record)
    with torch.no_grad():
        image = torch.empty(1, 3, H, W, device="meta")
        feats = fs(*fe(image))
        skips_and_bottom = enc(*feats, torch.empty(1, 64, H // 2, W // 2, device="meta"))
        dec(image, *skips_and_bottom)
        lstm.lstm_cell.conv(torch.empty(1, 1024, H // 32, W // 32, device="meta"))
    return seen


@pytest.mark.parametrize("size", cases.SIZES, ids=cases.size_id)
def test_the_layer_tables_are_the_networks_layers(size):
    W, H = size
    traced = traced_layers(W, H)
    dense = {p[:6] for p in traced if p[6] == 1 and p[4] in (3, 5) and p[1] > 1 and p[:2] != cases.LSTM_PROBLEM}
    assert sorted(dense) == cases.dense_problems(W, H)
    assert sorted(p[:4] for p in traced if p[6] == 1 and p[4] == 1) == cases.pointwise_problems(W, H)
    assert sorted((p[0], p[2], p[3]) for p in traced if p[6] == 1 and p[4] == 3 and p[1] == 1) == cases.EXPECTED[size]["head"]
    assert [p for p in traced if p[:2] == cases.LSTM_PROBLEM] == [cases.LSTM_PROBLEM + (H // 32, W // 32, 3, 1, 1)]
    assert all(p[6] == p[0] == p[1] for p in traced if p[6] != 1)      # everything else is depthwise: its own kernel at every size


# ---- the shape rules give the expected lists ---------------------------------------------------------------------------------------------------
def derived(W, H):
    """The size's problem lists from the layer tables and the library's shape rules, asked in FusedConv2d._forward's order: bottleneck kernel,
    direct kernel, pointwise kernel, else the library."""
    out = {"bottleneck": [], "direct": [], "pointwise": [], "library": []}
    for ci, co, h, w, k, s in cases.dense_problems(W, H):
        if k == 3 and lib().dvmvs_bottleneck_conv_splits(1, co, ci, h, w, s) > 0:
            out["bottleneck"].append((ci, co, h, w, s))
        elif lib().dvmvs_direct_conv_shape(1, ci, h, w, co, k, s) != 0:
            out["direct"].append((ci, h, w, co, k, s))
        else:
            out["library"].append((ci, co, h, w, k, s))
    for ci, co, d in cases.POINTWISE_LAYERS:
        h, w, mode = H // d, W // d, 2 if (ci, co, d) in cases.POINTWISE_ADDS_COARSER else 0
        assert lib().dvmvs_direct_conv_shape(1, ci, h, w, co, 1, 1) == 0      # (asked first: it takes no 1x1 layer)
        # (ReLU or none, a same-shape residual or none: the rule does not tell them apart; the lateral layers' up-sampled residual it does)
        taken = lib().dvmvs_pointwise_conv_supported(1, ci, h, w, co, 0, mode)
        assert taken == lib().dvmvs_pointwise_conv_supported(1, ci, h, w, co, 1, mode) and (mode or taken == lib().dvmvs_pointwise_conv_supported(1, ci, h, w, co, 1, 1))
        out["pointwise" if taken else "library"].append((ci, co, h, w) if taken else (ci, co, h, w, 1, 1))
    out = {k: sorted(v) for k, v in out.items()}
    out["lstm"] = ["bottleneck" if lib().dvmvs_bottleneck_conv_splits(1, 2048, 1024, H // 32, W // 32, 1) > 0 else "library"]
    return out


@pytest.mark.parametrize("size", cases.SIZES, ids=cases.size_id)
def test_the_shape_rules_give_the_expected_problem_lists(size):
    got, expected = derived(*size), cases.EXPECTED[size]
    for kind in got:
        assert got[kind] == expected[kind], (size, kind)
    # the facts that tell the sizes apart
    assert (expected["lstm"] == ["bottleneck"]) == (size in ((320, 256), (640, 512)))
    assert (not expected["bottleneck"] and not expected["direct"]) == (size in ((96, 64), (256, 256)))
    assert lib().dvmvs_bottleneck_conv_splits(1, 2048, 1024, 16, 20, 1) == 32 and lib().dvmvs_bottleneck_conv_splits(1, 2048, 1024, 8, 10, 1) == 16


# ---- every problem has a kernel-level pin ------------------------------------------------------------------------------------------------------
def test_every_bottleneck_problem_is_pinned():
    import test_bottleneck_conv_gpu as bc
    pinned = set(bc.SHAPES)
    for size in cases.SIZES:
        for problem in cases.EXPECTED[size]["bottleneck"]:
            assert problem in pinned, (size, problem)
        if cases.EXPECTED[size]["lstm"] == ["bottleneck"]:
            assert cases.LSTM_PROBLEM + (size[1] // 32, size[0] // 32, 1) in pinned, size
    assert (1024, 2048, 16, 20, 1) in bc.BATCH_ONE_ONLY


def test_every_direct_problem_runs_a_pinned_kernel():
    pinned = {(lib().dvmvs_direct_conv_shape(*case), case[5], case[6]) for case in dc.CASES}
    reached = set()
    for size in cases.SIZES:
        for ci, h, w, co, k, s in cases.EXPECTED[size]["direct"]:
            variant = (lib().dvmvs_direct_conv_shape(1, ci, h, w, co, k, s), k, s)
            assert variant[0] != 0 and variant in pinned, (size, (ci, h, w, co, k, s), variant)
            reached.add(variant)
    print(f"direct-convolution kernels the five sizes run: {sorted(reached)}")
    assert {(1, 3, 1), (1, 3, 2), (2, 5, 2)} <= reached      # (what no 320x256 frame runs)


def test_the_pointwise_test_takes_its_size_shapes_from_the_lists():
    """tests/test_pointwise_conv_gpu.py computes SIZE_SHAPES and SIZE_LATERAL_SHAPES from engine_size_cases.EXPECTED, so this holds by construction:
    it fails only if those lists are replaced by literals that drift."""
    import test_pointwise_conv_gpu as pw
    pinned = set(pw.FRAME_SHAPES) | set(pw.SIZE_SHAPES) | set(pw.RAGGED_SHAPES)
    for size in cases.SIZES:
        for problem in cases.EXPECTED[size]["pointwise"]:
            assert problem in pinned, (size, problem)
        for problem in cases.lateral_problems(*size):      # the layers whose epilogue adds the up-sampled coarser level: pinned with that residual
            assert problem in set(pw.LATERAL_SHAPES) | set(pw.SIZE_LATERAL_SHAPES), (size, problem)


def test_depth_head_channels_and_kernel_forms_are_pinned():
    """The head kernel takes any map (one form below 16 384 pixels, one from there on) and any channel count.  Pinned as they are: the 320x256
    frame's heads, 640x512's widest and its full-resolution one (the two shapes the issue names).  Of the other sizes' heads only the channel
    count and the kernel form are pinned somewhere -- a weak statement, not a pin of every head problem."""
    import test_direct_conv_gpu as dcg
    pinned = set(dcg.HEAD_SHAPES)
    assert set(cases.EXPECTED[(320, 256)]["head"]) <= pinned and {(256, 32, 40), (32, 512, 640)} <= pinned
    channels, forms = {p[0] for p in pinned}, {p[1] * p[2] >= 16384 for p in pinned}
    for size in cases.SIZES:
        for ci, h, w in cases.EXPECTED[size]["head"]:
            assert ci in channels and (h * w >= 16384) in forms, (size, (ci, h, w))


# ---- the generator reproduces the smallest fixture -----------------------------------------------------------------------------------------------
def test_the_generator_reproduces_the_smallest_fixture(golden_dir):
    """The fixture holds float32 roundings, so what is asserted per value is |stored - regenerated float64| <= 2^-24 |v| (the rounding, 6e-8
    relative) + 1e-12 max(|v|, the tensor's mean magnitude): the stored number is the float32 nearest to a value within 1e-12 of the regenerated
    one.  Yardsticks within a factor of 2."""
    spec = importlib.util.spec_from_file_location("make_engine_size_goldens", os.path.join(golden_dir, "make_engine_size_goldens.py"))
    generator = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(generator)
    W, H = cases.SIZES[0]
    z = cases.load_fixture(W, H, golden_dir)
    arrays, exact = generator.size_arrays(W, H, state_from=z)
    assert sorted(arrays) == sorted(z)
    for name, values in exact.items():
        stored = z[name].astype(np.float64)
        assert stored.shape == values.shape, name
        # 1e-12 of the value or of the tensor's mean magnitude (another thread count moves the float64 pipeline by 1e-13 of it, measured)
        allowed = np.abs(values) * 2.0 ** -24 + 1e-12 * np.maximum(np.abs(values), np.mean(np.abs(values)))
        assert bool(np.all(np.abs(stored - values) <= allowed)), (name, float(np.max(np.abs(stored - values) / np.mean(np.abs(values)))))
    for name in z:
        if name.endswith("_yardstick"):
            assert 0.5 * float(z[name]) <= float(arrays[name]) <= 2.0 * float(z[name]), (name, float(arrays[name]), float(z[name]))
        elif name.endswith("64_sum"):      # (the whole tensor, not only its samples)
            assert abs(float(arrays[name]) - float(z[name])) <= 1e-9 * float(z.get(name[:-3] + "abs_sum", z[name])), name      # (depth: its own sum)
        elif name.endswith("_depth_estimation"):
            assert cases.flipped_pixels(arrays[name], z[name]) == 0, name
        elif name.endswith("_estimate_flips"):
            assert int(arrays[name]) == int(z[name]) == 0
    assert all(z[f"f{n}_state_{k}"].dtype == (np.float16 if k == "depth_q" else np.int8) for n in (1, 2) for k in ("h_q", "c_q", "depth_q"))

"""tests/frame_reference.py pinned on the CPU, so that the GPU tests of the frame-path kernels (tests/test_frame_kernels_gpu.py) do not
rest on an unchecked reference: its float32 results are the plain ATen expressions the older tests use (bit for bit where those are
single ops) and what the product's CPU modules compute, its float64 results are the same algebra, and four answers are computed by
hand.  The references of the recurrent chain (gates, gates on partial sums, hidden-state warp: tests/test_state_kernels_gpu.py) are the
oracle bit for bit in float32 and ATen's LayerNorm / CELU / grid_sample in float64; the warp cases of tests/state_cases.py are proven
here to hold the geometry classes they are built for."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dvmvs_oracle as orc
import frame_reference as fr
import state_cases as sc
import synthetic as syn


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


ATEN_ACT = {fr.ACT_NONE: lambda t: t, fr.ACT_RELU: torch.relu, fr.ACT_SIGMOID: torch.sigmoid}


# ----------------------------------------------------------------------------------------------------------------------
# float32 = the ATen expressions of tests/test_hip_parity.py, tests/test_training_ops_gpu.py, tests/test_bottleneck_conv_gpu.py
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 7, 6, 4), (1, 3, 5, 3), (3, 2, 8, 10)])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_bias_act_is_the_aten_expression(shape, act):
    x, b, r = _rand(*shape, seed=1), _rand(shape[1], seed=2), _rand(*shape, seed=3)
    exp = ATEN_ACT[act](x + b.view(1, -1, 1, 1))
    assert torch.equal(fr.bias_act(x, b, act), exp)
    assert torch.equal(fr.bias_act(x, None, act), ATEN_ACT[act](x))
    assert torch.equal(fr.bias_act(x, b, act, r, fr.RES_SAME), exp + r)
    if shape[2] % 2 == 0 and shape[3] % 2 == 0:
        rh = _rand(shape[0], shape[1], shape[2] // 2, shape[3] // 2, seed=4)
        assert torch.equal(fr.bias_act(x, b, act, rh, fr.RES_NEAREST_UP2), exp + F.interpolate(rh, size=shape[2:], mode="nearest"))
    assert fr.bias_act(x, b, act, r, fr.RES_SAME, dtype=torch.float64).dtype == torch.float64


def test_depth_mapping_is_the_decoders_expression():
    """fusionnet/model.py: depth = 1 / (multiplier * sigmoid(conv + bias) + base); the parameters are the float32 values a kernel gets."""
    y, b = _rand(1, 1, 12, 20, seed=5, scale=3.0), _rand(1, seed=6)
    mult, base = 1 / 0.25 - 1 / 20.0, 1 / 20.0
    exp = 1.0 / (mult * torch.sigmoid(y + b.view(1, 1, 1, 1)) + base)
    assert torch.equal(fr.bias_act(y, b, fr.ACT_SIGMOID_TO_DEPTH, p0=mult, p1=base), exp)
    m32, b32 = float(torch.tensor(mult, dtype=torch.float32)), float(torch.tensor(base, dtype=torch.float32))
    exp64 = 1.0 / (m32 * torch.sigmoid(y.double() + b.double().view(1, 1, 1, 1)) + b32)
    assert torch.equal(fr.bias_act(y, b, fr.ACT_SIGMOID_TO_DEPTH, p0=mult, p1=base, dtype=torch.float64), exp64)
    assert float(exp64.max()) <= 1 / b32 and float(exp64.min()) >= 1 / (m32 + b32)       # the depth range [0.25, 20]
    r = _rand(1, 1, 12, 20, seed=7)
    assert torch.equal(fr.bias_act(y, b, 3, r, fr.RES_SAME, p0=mult, p1=base), exp + r)


def test_nearest_residual_known_answer():
    x = torch.zeros(1, 1, 2, 4)
    rh = torch.tensor([[[[1.0, 2.0]]]])
    assert fr.bias_act(x, None, 0, rh, fr.RES_NEAREST_UP2).tolist() == [[[[1.0, 1.0, 2.0, 2.0], [1.0, 1.0, 2.0, 2.0]]]]


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 4, 1, 1), (1, 2, 1, 6), (1, 2, 6, 1), (1, 5, 8, 10)])
def test_upsample2x_is_aten_and_the_products_cpu_module(shape):
    from dvmvs.networks import _upsample2
    x, pb = _rand(*shape, seed=8, scale=2.0), _rand(shape[1], seed=9)
    aten = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
    assert torch.equal(fr.upsample2x(x), aten) and torch.equal(_upsample2(x), aten)
    assert torch.equal(fr.upsample2x(x, pb, fr.ACT_NONE), aten)          # a bias without a pre-activation is not applied
    for act in (1, 2):
        exp = F.interpolate(ATEN_ACT[act](x + pb.view(1, -1, 1, 1)), scale_factor=2, mode="bilinear", align_corners=True)
        assert torch.equal(fr.upsample2x(x, pb, act), exp)
        assert torch.equal(fr.upsample2x(x, None, act), F.interpolate(ATEN_ACT[act](x), scale_factor=2, mode="bilinear", align_corners=True))
    with pytest.raises(ValueError):
        fr.upsample2x(x, pb, 3)


def test_upsample2x_known_answer():
    """2x2 -> 4x4 with align_corners: the output pixel (i, j) samples the source at (i / 3, j / 3); bilinear interpolation reproduces the
    plane f(y, x) = 6 y + 3 x that the four corners 0, 3, 6, 9 lie on: out[i][j] = 2 i + j."""
    x = torch.tensor([[[[0.0, 3.0], [6.0, 9.0]]]])
    want = torch.tensor([[[[0.0, 1, 2, 3], [2, 3, 4, 5], [4, 5, 6, 7], [6, 7, 8, 9]]]], dtype=torch.float64)
    assert float((fr.upsample2x(x, dtype=torch.float64) - want).abs().max()) <= 1e-14
    assert float((fr.upsample2x(x).double() - want).abs().max()) <= 2e-6
    # relu(x - 4.5) = 0, 0, 1.5, 4.5: rows 0 and 3 of the output are the rows of the activated map, interpolated at j / 3
    got = fr.upsample2x(x, torch.tensor([-4.5]), fr.ACT_RELU, dtype=torch.float64)[0, 0]
    assert float((got[0] - torch.zeros(4, dtype=torch.float64)).abs().max()) <= 1e-14
    assert float((got[3] - torch.tensor([1.5, 2.5, 3.5, 4.5], dtype=torch.float64)).abs().max()) <= 1e-14
    assert float((got[1] - got[3] / 3).abs().max()) <= 1e-14 and float((got[2] - 2 * got[3] / 3).abs().max()) <= 1e-14


@pytest.mark.parametrize("k,stride", [(3, 1), (3, 2), (5, 1), (5, 2)])
@pytest.mark.parametrize("shape", [(2, 6, 9, 7), (1, 3, 2, 1), (1, 4, 8, 10)])
def test_depthwise_is_aten_and_the_products_cpu_module(k, stride, shape):
    from dvmvs.backbone import DepthwiseConv2d
    B, C, H, W = shape
    x, w, b, pb = _rand(*shape, seed=10), _rand(C, 1, k, k, seed=11, scale=0.3), _rand(C, seed=12), _rand(C, seed=13)
    for act in (0, 1, 2):
        assert torch.equal(fr.depthwise(x, w, b, stride, act), ATEN_ACT[act](F.conv2d(x, w, b, stride=stride, padding=k // 2, groups=C)))
    assert torch.equal(fr.depthwise(x, w, None, stride), F.conv2d(x, w, None, stride=stride, padding=k // 2, groups=C))
    layer = DepthwiseConv2d(C, C, k, padding=k // 2, stride=stride, groups=C, bias=False)
    with torch.no_grad():
        layer.weight.copy_(w)
        assert torch.equal(fr.depthwise(x, w, None, stride), layer(x))
    # pre-activated: "activate, then convolve with zero padding" -- the padding is written out here, so it cannot be activated by mistake
    # (a convolution of another shape: ATen may add in another order, so float64 decides and float32 is held to its round-off)
    for bias_in in (pb, None):
        for dtype, bound in ((torch.float64, 1e-14), (torch.float32, 2e-6)):
            a = torch.relu(x.to(dtype) + pb.to(dtype).view(1, -1, 1, 1)) if bias_in is not None else torch.relu(x.to(dtype))
            exp = torch.relu(F.conv2d(F.pad(a, (k // 2,) * 4, value=0.0), w.to(dtype), b.to(dtype), stride=stride, padding=0, groups=C))
            got = fr.depthwise(x, w, b, stride, fr.ACT_RELU, bias_in, True, dtype=dtype)
            assert got.shape == exp.shape and float((got - exp).abs().max()) <= bound * max(1.0, float(exp.abs().max()))
    assert torch.equal(fr.depthwise(x, w, b, stride, 0, pb, False), fr.depthwise(x, w, b, stride, 0))       # pre_bias alone: no effect


def test_depthwise_known_answers():
    """3x3 at stride 2 on a 3x3 map (odd size): the outputs are centred on the four corners.  With x = 1..9 row by row and
    w = [[1,10,-1],[2,20,-2],[3,30,-3]] (cross-correlation, zero padding):
      (0,0): 20*1 - 2*2 + 30*4 - 3*5 = 121      (0,1): 2*2 + 20*3 + 3*5 + 30*6 = 259
      (1,0): 10*4 - 1*5 + 20*7 - 2*8 = 159      (1,1): 1*5 + 10*6 + 2*8 + 20*9 = 261"""
    x = torch.arange(1.0, 10.0).view(1, 1, 3, 3)
    w = torch.tensor([[1.0, 10, -1], [2, 20, -2], [3, 30, -3]]).view(1, 1, 3, 3)
    for dtype in (torch.float32, torch.float64):
        assert fr.depthwise(x, w, None, 2, dtype=dtype).tolist() == [[[[121.0, 259.0], [159.0, 261.0]]]]
    assert fr.depthwise(x, w, torch.tensor([-200.0]), 2, fr.ACT_RELU).tolist() == [[[[0.0, 59.0], [0.0, 61.0]]]]
    # the zero padding stays zero under the pre-activation: x = -1 everywhere, pre_bias 2 -> every in-bounds tap is relu(1) = 1, and
    # an all-ones 3x3 kernel counts the in-bounds taps (4 in a corner, 6 on an edge, 9 inside); an activated padding would add relu(2)
    ones = torch.ones(1, 1, 3, 3)
    got = fr.depthwise(-torch.ones(1, 1, 4, 3), ones, None, 1, 0, torch.tensor([2.0]), True)
    assert got.tolist() == [[[[4.0, 6.0, 4.0], [6.0, 9.0, 6.0], [6.0, 9.0, 6.0], [4.0, 6.0, 4.0]]]]


@pytest.mark.parametrize("S", [1, 2, 7, 9])
def test_partial_sums_add_in_ascending_order(S):
    parts, bias = _rand(S, 2, 5, 3, 4, seed=14, scale=100.0), _rand(5, seed=15)
    got = parts[0].clone()
    for s in range(1, S):
        got += parts[s]
    assert torch.equal(fr.partial_sums(parts), got)
    assert torch.equal(fr.partial_sums(parts, bias, fr.ACT_RELU), torch.relu(got + bias.view(1, -1, 1, 1)))
    with pytest.raises(ValueError):
        fr.partial_sums(parts, bias, fr.ACT_SIGMOID)
    if S == 9:      # the order matters in float32, so that "ascending" is a statement a test can check
        assert not torch.equal(fr.partial_sums(parts), fr.partial_sums(parts.flip(0)))
    assert float((fr.partial_sums(parts, bias, 1, dtype=torch.float64) - torch.relu(parts.double().sum(0) + bias.double().view(1, -1, 1, 1))).abs().max()) <= 1e-12


# ----------------------------------------------------------------------------------------------------------------------
# float64 is the same algebra, and the gradients are those of ATen's ops
# ----------------------------------------------------------------------------------------------------------------------
def test_float32_and_float64_agree_to_float32_round_off():
    x, b, r = _rand(2, 4, 6, 8, seed=16), _rand(4, seed=17), _rand(2, 4, 6, 8, seed=18)
    w, parts = _rand(4, 1, 5, 5, seed=19, scale=0.2), _rand(5, 2, 4, 6, 8, seed=20)
    pairs = [(fr.bias_act, (x, b, 2, r, 1)), (fr.upsample2x, (x, b, 2)), (fr.depthwise, (x, w, b, 2, 1, b, True)), (fr.partial_sums, (parts, b, 1))]
    for fn, args in pairs:
        lo, hi = fn(*args), fn(*args, dtype=torch.float64)
        assert lo.dtype == torch.float32 and hi.dtype == torch.float64 and lo.shape == hi.shape
        assert float((lo.double() - hi).abs().max()) <= 1e-5 * max(1.0, float(hi.abs().max()))


def test_gradients_are_autograd_of_the_aten_ops():
    x, w = _rand(2, 3, 5, 4, seed=21), _rand(3, 1, 3, 3, seed=22)
    gu, gd = _rand(2, 3, 10, 8, seed=23), _rand(2, 3, 3, 2, seed=24)
    x64 = x.double().requires_grad_(True)
    F.interpolate(x64, scale_factor=2, mode="bilinear", align_corners=True).backward(gu.double())
    (g,) = fr.gradients(fr.upsample2x, (x,), gu, dtype=torch.float64)
    assert torch.equal(g, x64.grad)
    # the adjoint identity <up(x), g> = <x, up^T g>
    assert abs(float((fr.upsample2x(x, dtype=torch.float64) * gu.double()).sum() - (x.double() * g).sum())) <= 1e-10
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    F.conv2d(x64, w64, padding=1, stride=2, groups=3).backward(gd.double())
    gx, gw = fr.gradients(lambda a, b, dtype: fr.depthwise(a, b, None, 2, dtype=dtype), (x, w), gd, dtype=torch.float64)
    assert torch.equal(gx, x64.grad) and torch.equal(gw, w64.grad)
    gx32, gw32 = fr.gradients(lambda a, b, dtype: fr.depthwise(a, b, None, 2, dtype=dtype), (x, w), gd)
    assert gx32.dtype == torch.float32 and float((gx32.double() - gx).abs().max()) <= 1e-5 and float((gw32.double() - gw).abs().max()) <= 1e-4


# ----------------------------------------------------------------------------------------------------------------------
# the recurrent chain: float32 = the oracle bit for bit, float64 = ATen's own ops, the fixtures of tests/golden
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", sc.GATE_MAPS)
def test_lstm_gates_is_the_oracle_and_aten(H, W):
    B, hid = 3, 5
    cc, c = sc.gate_inputs(B, hid, H, W, seed=100 + H * W)
    h, cn = fr.lstm_gates(cc, c)
    eh, ec = orc.lstm_gates(cc, c)
    assert h.dtype == torch.float32 and torch.equal(h, eh) and torch.equal(cn, ec)
    # float64: torch's own LayerNorm, CELU and sigmoid
    cc64, c64 = cc.double(), c.double()
    i, f, o, g = torch.split(cc64, hid, dim=1)
    c_next = F.layer_norm(torch.sigmoid(f) * c64 + torch.sigmoid(i) * F.celu(F.layer_norm(g, [H, W], eps=1e-5)), [H, W], eps=1e-5)
    h64, cn64 = fr.lstm_gates(cc, c, dtype=torch.float64)
    assert h64.dtype == torch.float64
    assert float((cn64 - c_next).abs().max()) <= 1e-12 and float((h64 - torch.sigmoid(o) * F.celu(c_next)).abs().max()) <= 1e-12


@pytest.mark.parametrize("kind", ["narrow", "saturated"])
def test_lstm_gates_hard_values_are_the_oracle(kind):
    cc, c = sc.hard_gate_inputs(kind, 2, 5, 8, 10, seed=400)
    for got, exp in zip(fr.lstm_gates(cc, c), orc.lstm_gates(cc, c)):
        assert torch.isfinite(got).all() and torch.equal(got, exp)


def test_lstm_gates_known_answer():
    """A 1x2 plane, one channel, by hand: LN(g = (1, 3)) = (-a, a) with a = 1 / sqrt(1 + 1e-5); i = f = o = 0 make every sigmoid 1/2
    and c = 0, so z = celu(LN g) / 2 = (expm1(-a), a) / 2, c' = LN(z) and h' = celu(c') / 2."""
    a = 1.0 / math.sqrt(1.0 + 1e-5)
    z = torch.tensor([math.expm1(-a), a], dtype=torch.float64) / 2
    want_c = (z - z.mean()) / torch.sqrt(((z - z.mean()) ** 2).mean() + 1e-5)
    want_h = 0.5 * torch.where(want_c > 0, want_c, torch.expm1(want_c))
    cc = torch.tensor([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 3.0]).view(1, 4, 1, 2)
    h, cn = fr.lstm_gates(cc, torch.zeros(1, 1, 1, 2), dtype=torch.float64)
    assert float((cn.view(-1) - want_c).abs().max()) <= 1e-14 and float((h.view(-1) - want_h).abs().max()) <= 1e-14
    assert float(cn.view(-1)[0]) < 0 < float(cn.view(-1)[1])


@pytest.mark.parametrize("S", [1, 2, 5, 6, 16])
def test_lstm_gates_partials_add_in_ascending_order(S):
    parts, c = _rand(S, 2, 20, 8, 10, seed=30 + S, scale=1.5 / S ** 0.5), _rand(2, 5, 8, 10, seed=31)
    total = parts[0].clone()
    for s in range(1, S):
        total += parts[s]
    for got, exp in zip(fr.lstm_gates_partials(parts, c), orc.lstm_gates(total, c)):
        assert torch.equal(got, exp)
    for got, exp in zip(fr.lstm_gates_partials(parts, c, dtype=torch.float64), fr.lstm_gates(parts.double().sum(0), c, dtype=torch.float64)):
        assert got.dtype == torch.float64 and float((got - exp).abs().max()) <= 1e-12
    if S == 1:
        assert all(torch.equal(a, b) for a, b in zip(fr.lstm_gates_partials(parts, c), fr.lstm_gates(parts[0], c)))


@pytest.mark.parametrize("kind", sc.WARP_KINDS)
@pytest.mark.parametrize("shape", sc.WARP_SHAPES + [sc.WARP_GRID_STRIDE_SHAPE])
def test_hidden_warp_is_the_oracle_and_grid_sample(shape, kind):
    """float32: oracle.warp_hidden_state bit for bit, masked and not.  float64: F.grid_sample fed the same normalised grid.  And the
    case holds its geometry class and the |z| > 0.05 precondition (what tests/test_state_kernels_gpu.py relies on)."""
    B, C, H, W = shape
    C = min(C, 3)
    depth, T, K = sc.warp_case(kind, B, H, W, seed=900 + H * W)
    src = _rand(B, C, H, W, seed=40)
    for mask in (False, True):
        out, ix, iy, z = fr.hidden_warp(src, depth, T, K, mask)
        assert out.dtype == torch.float32 and ix.dtype == iy.dtype == z.dtype == torch.float64 and tuple(z.shape) == (B, H, W)
        assert torch.equal(out, orc.warp_hidden_state(src, depth, T, K, zero_invalid=mask))
    sc.check_warp_case(kind, depth, ix, iy, z, H, W)
    out64, ix64, iy64, z64 = fr.hidden_warp(src, depth, T, K, False, dtype=torch.float64)
    assert torch.equal(ix64, ix) and torch.equal(iy64, iy) and torch.equal(z64, z)
    grid, _ = fr.warp_grid(depth, T, K, torch.float64)
    aten = F.grid_sample(src.double(), grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    assert float((out64 - aten).abs().max()) <= 1e-12
    masked64 = fr.hidden_warp(src, depth, T, K, True, dtype=torch.float64)[0]
    gone = (depth <= torch.tensor(0.01, dtype=torch.float32)).expand(B, C, H, W)
    assert float(masked64[gone].abs().max() if gone.any() else 0.0) == 0.0 and torch.equal(masked64[~gone], out64[~gone])
    if kind != "shift" and kind != "borders":        # 0 and 0.01f are masked, the next float is not
        zero, edge, above = sc.special_depths()
        assert bool(gone[(depth == edge).expand_as(gone)].all()) and not bool(gone[(depth == above).expand_as(gone)].any())


def test_hidden_warp_shift_known_answer():
    """A pure shift by (1.5, -0.5) pixels: out(y, x) = the mean of the four source pixels around (x + 1.5, y - 0.5), missing ones 0."""
    depth, T, K = sc.warp_case("shift", 1, 4, 5, seed=1)
    src = torch.arange(20.0).view(1, 1, 4, 5)
    out = fr.hidden_warp(src, depth, T, K, dtype=torch.float64)[0][0, 0]
    padded = F.pad(src.double()[0, 0], (0, 3, 1, 0))                 # one zero row above, three zero columns to the right
    want = (padded[0:4, 1:6] + padded[0:4, 2:7] + padded[1:5, 1:6] + padded[1:5, 2:7]) / 4
    assert float((out - want).abs().max()) <= 1e-5


def test_recurrent_fixtures_of_the_reference_run(golden_dir):
    """tests/golden/hidden_warp.npz and lstm_gates.npz (captured from the reference) within the tolerances tests/test_hip_parity.py
    uses for the kernels: 5e-6 for the warp, 1e-5 for the gates."""
    z = np.load(os.path.join(golden_dir, "hidden_warp.npz"))
    lK = syn.scaled_K(syn.full_K(), 32.0)
    _, _, h0, c0 = syn.analytic_lstm_inputs()
    t = lambda k: torch.from_numpy(z[k])      # noqa: E731
    for depth, T, mask, want in (("depth", "T", False, "warped"), ("depth_masked", "T", True, "warped_masked"), ("depth", "T_far", False, "warped_far")):
        for dtype in (torch.float32, torch.float64):
            got = fr.hidden_warp(h0, t(depth), t(T), lK, mask, dtype=dtype)[0]
            assert float((got.double() - t(want).double()).abs().max()) < 5e-6, (want, dtype)
    z = np.load(os.path.join(golden_dir, "lstm_gates.npz"))
    o = np.arange(2048, dtype=np.float64).reshape(-1, 1, 1)
    yy, xx = np.arange(8, dtype=np.float64).reshape(1, -1, 1), np.arange(10, dtype=np.float64).reshape(1, 1, -1)
    cc = torch.from_numpy((2.0 * np.sin(0.013 * o + 0.7 * yy + 0.3 * xx) + 0.5 * np.cos(0.05 * o * xx)).astype(np.float32)).unsqueeze(0)
    for dtype in (torch.float32, torch.float64):
        h, c = fr.lstm_gates(cc, c0, dtype=dtype)
        assert float((h.double() - torch.from_numpy(z["h_next"]).double()).abs().max()) < 1e-5
        assert float((c.double() - torch.from_numpy(z["c_next"]).double()).abs().max()) < 1e-5

"""The small kernels every frame and every training step run between the convolutions -- csrc/frame_ops.hip (bias + activation,
x2 up-sampling alone and paired, depthwise convolution), csrc/train_ops.hip (up-sampler and depthwise gradients) and the partial-sum
epilogue of csrc/bottleneck_conv.hip -- on every path their launchers pick from shape, alignment and size.

The arbiter is float64: tests/frame_reference.py states each op once, its float32 call is ``ref32`` and its float64 call ``ref64``, and
every value comparison is ``accuracy.as_accurate_as_reference(got, ref32, ref64)`` with its defaults (slack 3, floor 2e-6) over ALL
elements -- these functions are continuous, so there is no exclusion rule.  The sigmoid -> depth activation reaches 1 / p1 = 20, so
there the three tensors are divided by ``ref64`` (relative error, same slack and floor).  Where a kernel promises more, the stronger
statement is asserted too: bias + none | ReLU is one IEEE add (= float32 bit for bit), the partial sums are the ascending float32 sum
bit for bit, the quad up-sampler equals the one-output kernel bit for bit, and every kernel here is atomics-free: a second launch
repeats bit for bit.  Destinations are carved out of canary-filled buffers; everything outside the written slice must keep the canary.

Each section's docstring lists the kernel's paths by the condition in the launcher that selects them, next to the case that takes
each.  Sections print the kernel's and the float32 reference's largest distance to float64 (run with -s to see them).
"""
import functools

import pytest
import torch

import frame_reference as fr
from accuracy import as_accurate_as_reference

pytestmark = pytest.mark.gpu

CANARY = -12345.0
PAD = 64                      # floats of canary in front of and behind every destination (a multiple of 4: keeps the alignment)
DEPTH_P0, DEPTH_P1 = 1 / 0.25 - 1 / 20.0, 1 / 20.0        # the decoder's inverse_depth_multiplier, inverse_depth_base
EINVAL, EUNSUPPORTED = -1, -2                             # include/dvmvs_hip.h

STATS = {}


@pytest.fixture(scope="module")
def dev(hip_device):
    from dvmvs.hip import _capi
    _capi.lib()  # the HIP library must be there: no fallback
    yield hip_device
    for section, (ek, er, n) in STATS.items():
        print(f"\n[frame kernels] {section}: {n} comparisons, max |kernel - float64| {ek:.2e} (float32 reference: {er:.2e})")


@pytest.fixture(scope="module")
def ops(dev):
    from dvmvs.hip import ops as o
    return o


@pytest.fixture(scope="module")
def lib(dev):
    from dvmvs.hip import _capi
    return _capi.lib()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


@functools.lru_cache(maxsize=None)
def _randn(shape, seed, scale=1.0):
    """Inputs are built once per (shape, seed), not once per parametrised activation."""
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _ptr(t):
    return None if t is None else t.data_ptr()


def check(section, got, ref32, ref64, relative=False, label=""):
    """The one value comparison of this module; ``relative`` divides all three by ref64 (activation 3 only)."""
    got = got.detach().cpu()
    assert got.shape == ref64.shape, (label, tuple(got.shape), tuple(ref64.shape))
    assert torch.isfinite(got).all(), label
    g, r32, r64 = got.double(), ref32.detach().double(), ref64.detach()
    if relative:
        g, r32, r64 = g / r64, r32 / r64, r64 / r64
    ek, er = float((g - r64).abs().max()), float((r32 - r64).abs().max())
    s = STATS.setdefault(section + (" (relative)" if relative else ""), [0.0, 0.0, 0])
    s[0], s[1], s[2] = max(s[0], ek), max(s[1], er), s[2] + 1
    print(f"{section} {label}: max |kernel - float64| {ek:.2e} (float32 reference: {er:.2e})")
    as_accurate_as_reference(g, r32, r64)


class Canvas:
    """A destination of B items of ``per_item`` floats, ``stride`` floats apart, ``offset`` floats into a 16-byte-aligned
    canary-filled buffer with PAD canaries on either side."""

    def __init__(self, dev, B, per_item, stride=None, offset=0):
        self.B, self.per, self.stride, self.start = B, per_item, per_item if stride is None else stride, PAD + offset
        self.buf = torch.full((self.start + (B - 1) * self.stride + per_item + PAD,), CANARY, device=dev)
        assert self.buf.data_ptr() % 16 == 0 and self.stride >= per_item

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * self.start

    def _items(self, t):
        return t.as_strided((self.B, self.per), (self.stride, 1), self.start)

    def read(self):
        return self._items(self.buf).clone()

    def outside_intact(self):
        rest = self.buf.clone()
        self._items(rest).fill_(CANARY)
        return bool((rest == CANARY).all())

    def untouched(self):
        return bool((self.buf == CANARY).all())


def place(dev, t, offset=0):
    """``t`` on the device, ``offset`` floats behind a 16-byte boundary (0: aligned); None stays None."""
    if t is None:
        return None
    buf = torch.empty(t.numel() + offset + 4, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + t.numel()]
    view.copy_(t.reshape(-1).to(dev))
    return view


# ----------------------------------------------------------------------------------------------------------------------
# up-sampler forward: dvmvs_upsample2x_fwd (frame_ops.hip, launcher at the end of the file)
# ----------------------------------------------------------------------------------------------------------------------
# destination layouts: (offset in floats, batch stride in floats) from (C, OH * OW)
LAYOUTS = {
    "dense": lambda C, P: (0, C * P),
    "slice": lambda C, P: (2 * P, (C + 3) * P),          # channels [2, 2 + C) of a [B, C + 3, OH, OW] buffer
    "misaligned": lambda C, P: (1, C * P),               # 4-byte aligned only
    "odd_stride": lambda C, P: (0, C * P + 2),           # batch stride & 3 != 0: only a caller of the C entry point can pass it
}


def takes_quads(ptr, stride, B, C, W):
    """The launcher's condition for upsample2x_quads_kernel (else upsample2x_kernel, one output per thread)."""
    return W % 2 == 0 and ptr % 16 == 0 and stride % 4 == 0 and B * C <= 65535


def run_upsample(lib, dev, x, pre_bias, pre, layout):
    B, C, H, W = x.shape
    offset, stride = LAYOUTS[layout](C, 4 * H * W)
    cv = Canvas(dev, B, C * 4 * H * W, stride, offset)
    xd, pb = x.to(dev), None if pre_bias is None else pre_bias.to(dev)
    outs = []
    for _ in range(2):
        cv.buf.fill_(CANARY)
        assert lib.dvmvs_upsample2x_fwd(xd.data_ptr(), cv.ptr, stride, _ptr(pb), pre, B, C, H, W, _stream(dev)) == 0
        torch.cuda.synchronize(dev)
        outs.append(cv.read().view(B, C, 2 * H, 2 * W))
        assert cv.outside_intact(), (tuple(x.shape), pre, layout)
    assert torch.equal(outs[0], outs[1]), "the up-sampler is not bit-reproducible"
    return outs[0], takes_quads(cv.ptr, stride, B, C, W)


def upsample_refs(x, pre_bias, pre):
    return fr.upsample2x(x, pre_bias, pre), fr.upsample2x(x, pre_bias, pre, dtype=torch.float64)


UPSAMPLE_CASES = [  # (shape, layout, quad path expected)
    ((1, 5, 16, 20), "dense", True),            # quad path: W even, destination and stride 16-byte aligned; B = 1, C > 1
    ((2, 3, 6, 8), "dense", True),              # ... B = 2 with a per-channel pre_bias: bias c of plane b * C + c
    ((2, 3, 6, 8), "slice", True),              # ... into a channel slice (stride (C + 3) * OH * OW)
    ((1, 4, 6, 8), "slice", True),
    ((2, 3, 1, 8), "dense", True),              # H = 1: sh = 0, both rows are row 0
    ((2, 3, 5, 7), "dense", False),             # one-output path by W % 2 != 0
    ((1, 4, 8, 5), "slice", False),
    ((2, 3, 6, 8), "misaligned", False),        # one-output path by (out & 15) != 0
    ((2, 3, 6, 8), "odd_stride", False),        # one-output path by (out_batch_stride & 3) != 0
    ((1, 2, 1, 5), "dense", False),             # H = 1, odd W
    ((2, 3, 6, 1), "dense", False),             # W = 1: sw = 0
    ((1, 4, 1, 1), "dense", False),             # (1, C, 1, 1): four copies of the (activated) input
]


@pytest.mark.parametrize("pre", [0, 1, 2])
@pytest.mark.parametrize("shape,layout,quads", UPSAMPLE_CASES)
def test_upsample_forward_paths(lib, dev, shape, layout, quads, pre):
    """Paths of dvmvs_upsample2x_fwd, each with pre-activation none (PRE 0), bias + ReLU (PRE 1), bias + sigmoid (PRE 2) on the taps:
    * upsample2x_quads_kernel<PRE>: ``W % 2 == 0 && (out & 15) == 0 && (out_batch_stride & 3) == 0 && B*C <= 65535``;
    * upsample2x_kernel<PRE> otherwise -- by odd W, by a 4-byte-aligned destination, by a batch stride of the dense size + 2 floats.
    The two kernels evaluate one expression per output, so an even-W case that is forced onto the one-output kernel must give the
    bits of the quad kernel."""
    x, pb = _randn(shape, 11, 2.0), _randn((shape[1],), 12)
    got, took_quads = run_upsample(lib, dev, x, pb, pre, layout)
    assert took_quads == quads
    check("upsample2x_fwd", got, *upsample_refs(x, pb, pre), label=f"{shape} {layout} pre={pre}")
    if pre == 0:
        no_bias, _ = run_upsample(lib, dev, x, None, pre, layout)
        assert torch.equal(no_bias, got)          # without a pre-activation pre_bias is not applied (include/dvmvs_hip.h)
    if layout in ("misaligned", "odd_stride"):
        quad, was_quad = run_upsample(lib, dev, x, pb, pre, "dense")
        assert was_quad and torch.equal(quad, got), "the quad kernel and the one-output kernel differ"


@pytest.mark.parametrize("pre", [0, 1, 2])
def test_upsample_forward_grid_stride_loops(lib, dev, pre):
    """* quad kernel's own loop: per_plane = max(1, min(ceil(quads / 256), max(1, 4096 / (B*C)))); at (2, 1040, 16, 20) B*C = 2080, so
      4096 / 2080 = 1 workgroup of 256 threads per plane for OH * OW/4 = 32 * 10 = 320 quads: 64 threads take a second quad;
    * one-output kernel's loop: the grid is capped at 4096 workgroups = 1 048 576 threads; (2, 8, 128, 161) (odd W) has
      16 * 256 * 322 = 1 318 912 outputs."""
    for shape, quads in (((2, 1040, 16, 20), True), ((2, 8, 128, 161), False)):
        B, C, H, W = shape
        assert (quads and 4096 // (B * C) == 1 and 2 * H * (W // 2) > 256) or (not quads and B * C * 4 * H * W > 4096 * 256)
        x, pb = _randn(shape, 13, 2.0), _randn((C,), 14)
        got, took_quads = run_upsample(lib, dev, x, pb, pre, "dense")
        assert took_quads == quads
        check("upsample2x_fwd", got, *upsample_refs(x, pb, pre), label=f"{shape} grid-stride pre={pre}")


def test_upsample_wrappers_reach_the_same_kernels(ops, lib, dev):
    """ops.upsample2x / ops.upsample2x_into (what the modules and the engine call) give the bits of the C entry point."""
    x, pb = _randn((2, 3, 6, 8), 11, 2.0), _randn((3,), 12)
    direct, _ = run_upsample(lib, dev, x, pb, 2, "dense")
    big = torch.full((2, 6, 12, 16), CANARY, device=dev)
    ops.upsample2x_into(x.to(dev), big[:, 2:5], pb.to(dev), ops.ACTIVATIONS["sigmoid"])
    assert torch.equal(big[:, 2:5], direct) and bool((big[:, :2] == CANARY).all()) and bool((big[:, 5:] == CANARY).all())
    plain, _ = run_upsample(lib, dev, x, None, 0, "dense")
    assert torch.equal(ops.upsample2x(x.to(dev)), plain)


# ----------------------------------------------------------------------------------------------------------------------
# pair launch: dvmvs_upsample2x_pair_fwd
# ----------------------------------------------------------------------------------------------------------------------
def run_pair(lib, dev, x1, x2, pb2, pre2, layout1, layout2):
    B, C1, H, W = x1.shape
    C2, P = x2.shape[1], 4 * H * W
    (o1, s1), (o2, s2) = LAYOUTS[layout1](C1, P), LAYOUTS[layout2](C2, P)
    cv1, cv2 = Canvas(dev, B, C1 * P, s1, o1), Canvas(dev, B, C2 * P, s2, o2)
    d1, d2, pb = x1.to(dev), x2.to(dev), None if pb2 is None else pb2.to(dev)
    outs = []
    for _ in range(2):
        cv1.buf.fill_(CANARY)
        cv2.buf.fill_(CANARY)
        rc = lib.dvmvs_upsample2x_pair_fwd(d1.data_ptr(), cv1.ptr, s1, C1, d2.data_ptr(), cv2.ptr, s2, _ptr(pb), pre2, C2, B, H, W, _stream(dev))
        assert rc == 0
        torch.cuda.synchronize(dev)
        outs.append((cv1.read().view(B, C1, 2 * H, 2 * W), cv2.read().view(B, C2, 2 * H, 2 * W)))
        assert cv1.outside_intact() and cv2.outside_intact()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "the pair launch is not bit-reproducible"
    one_launch = W % 2 == 0 and (cv1.ptr | cv2.ptr) % 16 == 0 and (s1 | s2) % 4 == 0 and B * (C1 + C2) <= 65535
    return outs[0], one_launch


def check_pair(lib, dev, shape, C1, C2, pre2, layout1, layout2, one_launch):
    B, H, W = shape
    x1, x2, pb2 = _randn((B, C1, H, W), 21), _randn((B, C2, H, W), 22, 2.0), _randn((C2,), 23)
    (got1, got2), took_one = run_pair(lib, dev, x1, x2, pb2, pre2, layout1, layout2)
    assert took_one == one_launch
    label = f"B={B} C1={C1} C2={C2} {H}x{W} {layout1}/{layout2} pre2={pre2}"
    check("upsample2x_pair_fwd", got1, *upsample_refs(x1, None, 0), label=label + " job 1")
    check("upsample2x_pair_fwd", got2, *upsample_refs(x2, pb2, pre2), label=label + " job 2")
    # "the same values bit for bit" as the two launches
    two1, _ = run_upsample(lib, dev, x1, None, 0, layout1)
    two2, _ = run_upsample(lib, dev, x2, pb2, pre2, layout2)
    assert torch.equal(got1, two1) and torch.equal(got2, two2)


@pytest.mark.parametrize("pre2", [0, 1, 2])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("C2", [1, 3])
@pytest.mark.parametrize("C1", [1, 32])
def test_pair_launch_one_kernel(lib, dev, C1, C2, B, pre2):
    """upsample2x_pair_quads_kernel<PRE2>: ``W % 2 == 0``, both destinations 16-byte aligned, both batch strides multiples of 4.  Planes
    [0, B*C1) are job 1 (never pre-activated), planes [B*C1, B*(C1+C2)) job 2 with pre_bias2[c] of ITS channel count C2; job 2 goes
    into a channel slice, as the decoder's depth head does."""
    check_pair(lib, dev, (B, 6, 8), C1, C2, pre2, "dense", "slice", True)


@pytest.mark.parametrize("pre2", [0, 1, 2])
@pytest.mark.parametrize("shape,layout1,layout2", [((2, 5, 7), "dense", "slice"), ((2, 6, 8), "dense", "misaligned"),
                                                   ((1, 6, 8), "slice", "odd_stride")])
def test_pair_launch_fallback(lib, dev, shape, layout1, layout2, pre2):
    """``!quads``: two dvmvs_upsample2x_fwd launches -- by odd W (both on the one-output kernel), by a misaligned dst2 only and by a dst2
    batch stride & 3 != 0 only (job 1 stays on the quad kernel, job 2 takes the one-output kernel with its pre-activation)."""
    check_pair(lib, dev, shape, 3, 2, pre2, layout1, layout2, False)


def test_pair_launch_grid_stride(lib, dev):
    """per_plane = max(1, min(ceil(quads / 256), 4096 / planes)): 2 * (1040 + 1) planes of 16 x 20 -> one workgroup for 320 quads."""
    check_pair(lib, dev, (2, 16, 20), 1040, 1, 2, "dense", "dense", True)


# ----------------------------------------------------------------------------------------------------------------------
# up-sampler gradient: dvmvs_upsample2x_bwd (train_ops.hip)
# ----------------------------------------------------------------------------------------------------------------------
UPSAMPLE_BWD_SHAPES = [(2, 3, 1, 1), (1, 2, 1, 7), (1, 2, 7, 1), (1, 2, 2, 3), (2, 3, 3, 2), (1, 2, 3, 1), (1, 3, 2, 2), (2, 3, 8, 10),
                       (1, 4, 33, 47), (4, 32, 96, 96)]


@pytest.mark.parametrize("shape", UPSAMPLE_BWD_SHAPES)
def test_upsample_gradient(ops, dev, shape):
    """upsample2x_bwd_kernel, one thread per INPUT element gathering the <= 6 x 6 outputs around (2y, 2x):
    * H or W in {1, 2, 3}: the window [2y - 2, 2y + 3] is cut by both borders, sh = 0 at H = 1, the clamped tap y1 = y0 at the end;
    * odd sizes, where the float32 source position sh * oy is inexact;
    * the grid-stride loop: the grid is capped at 4096 workgroups = 1 048 576 threads; (4, 32, 96, 96) has 1 179 648 input
      elements (training's last decoder level, 4 x 32 x 128 x 128, is the same path).
    Against float64 autograd through frame_reference.upsample2x, and bit-equal on repeat."""
    B, C, H, W = shape
    if shape == UPSAMPLE_BWD_SHAPES[-1]:
        assert B * C * H * W > 4096 * 256
    x, gout = _randn(shape, 31), _randn((B, C, 2 * H, 2 * W), 32)
    got = ops.upsample2x_bwd(gout.to(dev))
    (g32,) = fr.gradients(fr.upsample2x, (x,), gout)
    (g64,) = fr.gradients(fr.upsample2x, (x,), gout, dtype=torch.float64)
    check("upsample2x_bwd", got, g32, g64, label=str(shape))
    assert torch.equal(ops.upsample2x_bwd(gout.to(dev)), got), "the up-sampler gradient is not bit-reproducible"
    if B * C * H * W < 10000:      # through autograd of the forward op, as training reaches it
        xd = x.to(dev).requires_grad_(True)
        ops.upsample2x(xd).backward(gout.to(dev))
        assert torch.equal(xd.grad, got)


# ----------------------------------------------------------------------------------------------------------------------
# depthwise forward: dvmvs_depthwise_conv_fwd
# ----------------------------------------------------------------------------------------------------------------------
def run_depthwise(ops, dev, x, w, bias, stride, act, pre_bias, pre_relu):
    none = torch.empty(0, device=dev)
    args = (x.to(dev), w.to(dev), none if bias is None else bias.to(dev), stride, act, none if pre_bias is None else pre_bias.to(dev), pre_relu)
    got = ops.depthwise_conv(*args)
    assert torch.equal(ops.depthwise_conv(*args), got), "the depthwise convolution is not bit-reproducible"
    return got


def depthwise_refs(x, w, bias, stride, act, pre_bias, pre_relu):
    return (fr.depthwise(x, w, bias, stride, act, pre_bias, pre_relu), fr.depthwise(x, w, bias, stride, act, pre_bias, pre_relu, dtype=torch.float64))


def depthwise_problem(shape, k):
    C = shape[1]
    return _randn(shape, 41), _randn((C, 1, k, k), 42 + k, 0.3), _randn((C,), 43), _randn((C,), 44)


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("k,stride", [(3, 1), (3, 2), (5, 1), (5, 2)])
def test_depthwise_forward_templates(ops, dev, k, stride, act, with_bias):
    """depthwise_conv_kernel<K, ACT, PRE>: K in {3, 5} x ACT in {0, 1, 2} x PRE, stride a run-time argument, bias nullable; B = 2 with an
    odd 9 x 7 map (at stride 2 the last output is centred on the last row / column) and an even 8 x 10 one (the last row / column is
    reached by the kernel's last tap only).  PRE (bias + ReLU on the in-bounds taps, the padding stays zero) with and without pre_bias;
    pre_bias without pre_relu must change nothing."""
    for shape in ((2, 6, 9, 7), (2, 5, 8, 10)):
        x, w, b, pb = depthwise_problem(shape, k)
        bias = b if with_bias else None
        label = f"{shape} k={k} s={stride} act={act} bias={with_bias}"
        got = run_depthwise(ops, dev, x, w, bias, stride, act, None, False)
        check("depthwise_conv_fwd", got, *depthwise_refs(x, w, bias, stride, act, None, False), label=label)
        assert torch.equal(run_depthwise(ops, dev, x, w, bias, stride, act, pb, False), got), "pre_bias without pre_relu changed the result"
        for pre_bias in (pb, None):
            got = run_depthwise(ops, dev, x, w, bias, stride, act, pre_bias, True)
            check("depthwise_conv_fwd", got, *depthwise_refs(x, w, bias, stride, act, pre_bias, True), label=label + f" pre_relu pre_bias={pre_bias is not None}")


@pytest.mark.parametrize("k,stride", [(3, 1), (3, 2), (5, 1), (5, 2)])
@pytest.mark.parametrize("shape", [(1, 3, 1, 1), (2, 3, 2, 1), (1, 3, 1, 2), (2, 2, 2, 2), (1, 2, 1, 9), (1, 2, 3, 2)])
def test_depthwise_forward_maps_smaller_than_the_kernel(ops, dev, shape, k, stride):
    """H or W in {1, 2}: most taps of every output are padding."""
    x, w, b, pb = depthwise_problem(shape, k)
    for pre in (False, True):
        got = run_depthwise(ops, dev, x, w, b, stride, 1, pb, pre)
        check("depthwise_conv_fwd", got, *depthwise_refs(x, w, b, stride, 1, pb, pre), label=f"{shape} k={k} s={stride} pre={pre}")


@pytest.mark.parametrize("k,stride,shape", [(3, 1, (1, 3, 130, 131)), (5, 1, (2, 2, 130, 131)), (3, 2, (1, 3, 258, 261)), (5, 2, (2, 2, 258, 261))])
def test_depthwise_forward_grid_stride_loop(ops, dev, k, stride, shape):
    """grid.x = min(ceil(OH*OW / 256), 64): the loop runs for OH*OW > 16 384 -- 130 x 131 = 17 030 at stride 1, 129 x 131 = 16 899 at
    stride 2."""
    B, C, H, W = shape
    assert ((H - 1) // stride + 1) * ((W - 1) // stride + 1) > 64 * 256
    x, w, b, pb = depthwise_problem(shape, k)
    got = run_depthwise(ops, dev, x, w, b, stride, 1, pb, True)
    check("depthwise_conv_fwd", got, *depthwise_refs(x, w, b, stride, 1, pb, True), label=f"{shape} k={k} s={stride} grid-stride")


# ----------------------------------------------------------------------------------------------------------------------
# depthwise gradients: dvmvs_depthwise_conv_bwd (train_ops.hip)
# ----------------------------------------------------------------------------------------------------------------------
def weight_slices(B, C, OH, OW):
    """depthwise_weight_slices() of train_ops.hip, restated; checked below against dvmvs_depthwise_conv_bwd_workspace_bytes."""
    total = B * OH * OW
    return max(1, min(64, (1024 + C - 1) // C, total // 4096))


DEPTHWISE_BWD_CASES = [  # (shape, k, stride, slices, what)
    ((2, 6, 9, 7), 3, 1, 1, "slices == 1"),
    ((2, 6, 9, 7), 5, 2, 1, "slices == 1, odd sizes at stride 2"),
    ((2, 5, 8, 10), 3, 2, 1, "even sizes at stride 2: the last row / column is read through the last tap only"),
    ((1, 3, 2, 1), 5, 1, 1, "a map smaller than the kernel"),
    ((3, 8, 75, 75), 3, 1, 4, "total 16875 in 4 chunks of 4219: chunks straddle the 5625-pixel images, the last one is short"),
    ((3, 8, 75, 75), 5, 1, 4, "the same at k = 5"),
    ((3, 8, 153, 149), 3, 2, 4, "odd sizes at stride 2: total 3 * 77 * 75 = 17325 in 4 chunks of 4332, straddling, the last one short"),
    ((3, 8, 153, 149), 5, 2, 4, "the same at k = 5"),
    ((1, 3, 130, 131), 3, 1, 4, "data gradient's grid-stride loop: H*W = 17030 > 16384; one image cut into 4 chunks of 4258"),
    ((1, 3, 130, 131), 5, 2, 1, "data gradient's grid-stride loop at stride 2"),
    ((2, 3, 363, 365), 3, 1, 64, "the 64-slice cap: C <= 16, total 264990 >= 262144, chunks of 4141 straddle the images"),
]


@pytest.mark.parametrize("shape,k,stride,slices,what", DEPTHWISE_BWD_CASES)
def test_depthwise_gradients(ops, lib, dev, shape, k, stride, slices, what):
    """* data gradient (depthwise_bwd_data_kernel<K>): one thread per input pixel, grid.x = min(ceil(H*W / 256), 64) -- its loop runs
      for H*W > 16 384; at stride 2 only every other tap contributes (``ty % stride``) and ``oy < OH`` cuts the far border.  With
      padding k / 2 every input pixel is read by some output; on even sizes at stride 2 the last row / column is read through the last
      kernel tap only, on odd sizes the last output is centred on it: both are run.
    * weight gradient (depthwise_bwd_weight_kernel<K> + the reduce kernel): slices = clamp(min(ceil(1024 / C), B*OH*OW / 4096), 1, 64),
      each a chunk of ceil(total / slices) consecutive (b, pixel) -- one slice writes grad_weight directly, several go through the
      workspace and are added in order.
    need_input / need_weight alone: the other output is empty and the wanted one has the same bits."""
    B, C, H, W = shape
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    assert weight_slices(B, C, OH, OW) == slices
    assert lib.dvmvs_depthwise_conv_bwd_workspace_bytes(B, C, H, W, k, stride) == (4 * slices * C * k * k if slices > 1 else 0)
    if slices > 1:      # no chunk boundary falls on an image boundary, and the last chunk is shorter than the others
        chunk = -(-B * OH * OW // slices)
        assert all((s * chunk) % (OH * OW) != 0 for s in range(1, slices)) and slices * chunk > B * OH * OW
    x, w = _randn(shape, 51), _randn((C, 1, k, k), 52 + k, 1.0 / k)
    gout = _randn((B, C, OH, OW), 53)
    fn = lambda a, b, dtype: fr.depthwise(a, b, None, stride, dtype=dtype)      # noqa: E731
    gx32, gw32 = fr.gradients(fn, (x, w), gout)
    gx64, gw64 = fr.gradients(fn, (x, w), gout, dtype=torch.float64)
    xd, wd, gd = x.to(dev), w.to(dev), gout.to(dev)
    gx, gw = ops.depthwise_conv_bwd(gd, xd, wd, stride, True, True)
    label = f"{shape} k={k} s={stride} ({slices} slices)"
    check("depthwise_conv_bwd data", gx, gx32, gx64, label=label)
    check("depthwise_conv_bwd weight", gw, gw32, gw64, label=label)
    again_x, again_w = ops.depthwise_conv_bwd(gd, xd, wd, stride, True, True)
    assert torch.equal(again_x, gx) and torch.equal(again_w, gw), "the depthwise gradients are not bit-reproducible"
    only_x, no_w = ops.depthwise_conv_bwd(gd, xd, wd, stride, True, False)
    no_x, only_w = ops.depthwise_conv_bwd(gd, xd, wd, stride, False, True)
    assert no_w.numel() == 0 and no_x.numel() == 0 and torch.equal(only_x, gx) and torch.equal(only_w, gw)
    if B * C * H * W < 10000:      # through autograd of the training op
        xa, wa = xd.clone().requires_grad_(True), wd.clone().requires_grad_(True)
        y = ops.depthwise_conv_train(xa, wa, stride)
        check("depthwise_conv_fwd", y, fr.depthwise(x, w, None, stride), fr.depthwise(x, w, None, stride, dtype=torch.float64), label=label + " training forward")
        y.backward(gd)
        assert torch.equal(xa.grad, gx) and torch.equal(wa.grad, gw)


# ----------------------------------------------------------------------------------------------------------------------
# bias + activation: dvmvs_bias_act_fwd / dvmvs_bias_act_inplace
# ----------------------------------------------------------------------------------------------------------------------
def bias_act_problem(shape, act, mode):
    """Activation 3 is compared by relative error: its residual is |randn| >= 0 (chosen here, from the inputs alone), so that
    depth + residual stays above the smallest depth 0.25 and the division by ref64 is well conditioned."""
    B, C, H, W = shape
    x, bias = _randn(shape, 61, 3.0 if act == 3 else 1.0), _randn((C,), 62)
    res = None
    if mode == fr.RES_SAME:
        res = _randn(shape, 63)
    elif mode == fr.RES_NEAREST_UP2:
        res = _randn((B, C, H // 2, W // 2), 64)
    if res is not None and act == 3:
        res = res.abs()
    p0, p1 = (DEPTH_P0, DEPTH_P1) if act == 3 else (0.0, 0.0)
    return x, bias, res, p0, p1


def run_bias_act(lib, dev, x, bias, act, res, mode, p0, p1, x_off=0, dst_off=0, res_off=0, stride_extra=0, in_place=False):
    """Through the C entry point; returns the result and whether the launcher's float4 condition held."""
    B, C, H, W = x.shape
    per = C * H * W
    stride = per + stride_extra
    xd, bd, rd = place(dev, x, x_off), place(dev, bias), place(dev, res, res_off)
    cv = Canvas(dev, B, per, stride, dst_off)
    outs = []
    for _ in range(2):
        if in_place:
            cv.buf.fill_(CANARY)
            cv._items(cv.buf).copy_(x.reshape(B, per).to(dev))
            rc = (lib.dvmvs_bias_act_inplace(cv.ptr, _ptr(bd), _ptr(rd), mode, B, C, H, W, act, _stream(dev)) if act != 3 else
                  lib.dvmvs_bias_act_fwd(cv.ptr, cv.ptr, stride, _ptr(bd), _ptr(rd), mode, B, C, H, W, act, p0, p1, _stream(dev)))
            src_ptr = cv.ptr
        else:
            cv.buf.fill_(CANARY)
            rc = lib.dvmvs_bias_act_fwd(xd.data_ptr(), cv.ptr, stride, _ptr(bd), _ptr(rd), mode, B, C, H, W, act, p0, p1, _stream(dev))
            src_ptr = xd.data_ptr()
        assert rc == 0
        torch.cuda.synchronize(dev)
        outs.append(cv.read().view(B, C, H, W))
        assert cv.outside_intact()
    assert torch.equal(outs[0], outs[1]), "bias_act is not bit-reproducible"
    vec4 = ((H * W) % 4 == 0 and src_ptr % 16 == 0 and (0 if rd is None else rd.data_ptr()) % 16 == 0 and cv.ptr % 16 == 0 and
            stride % 4 == 0 and mode != 2)
    return outs[0], vec4


def check_bias_act(lib, dev, shape, act, mode, vec4, label, **how):
    x, bias, res, p0, p1 = bias_act_problem(shape, act, mode)
    got, took_vec4 = run_bias_act(lib, dev, x, bias, act, res, mode, p0, p1, **how)
    assert took_vec4 == vec4, label
    ref32 = fr.bias_act(x, bias, act, res, mode, p0, p1)
    ref64 = fr.bias_act(x, bias, act, res, mode, p0, p1, dtype=torch.float64)
    check("bias_act", got, ref32, ref64, relative=act == 3, label=f"{shape} act={act} res={mode} {label}")
    if act in (0, 1):
        assert torch.equal(got.cpu(), ref32), "bias + none | ReLU (+ residual) is IEEE adds: float32 bit for bit"
    return got


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_bias_act_float4_and_scalar_by_size(lib, dev, act, mode):
    """launch_bias_act: ``vec4 = HW % 4 == 0 && x, residual, dst 16-byte aligned && dst_batch_stride % 4 == 0 && residual_mode != 2``.
    * bias_act_kernel<ACT, true, RES> for RES in {0, 1}: (2, 3, 4, 6), everything aligned;
    * bias_act_kernel<ACT, false, 2>: the half-resolution residual always takes the scalar kernel (same shape);
    * bias_act_kernel<ACT, false, RES> by HW % 4 != 0: (2, 3, 5, 3) and (1, 2, 6, 5) for RES in {0, 1}; the half-resolution residual
      needs even H and W, which makes HW a multiple of 4, so it cannot meet this condition (odd sizes are refused, see below);
    * every case once more in place (dst == x; dvmvs_bias_act_inplace for activations 0..2), the same bits."""
    got = check_bias_act(lib, dev, (2, 3, 4, 6), act, mode, mode != 2, "aligned")
    same = check_bias_act(lib, dev, (2, 3, 4, 6), act, mode, mode != 2, "in place", in_place=True)
    assert torch.equal(got, same)
    if mode != 2:
        for shape in ((2, 3, 5, 3), (1, 2, 6, 5)):
            check_bias_act(lib, dev, shape, act, mode, False, "HW % 4 != 0")
            check_bias_act(lib, dev, shape, act, mode, False, "HW % 4 != 0, in place", in_place=True)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_bias_act_scalar_by_alignment(lib, dev, act, mode):
    """HW % 4 == 0, but one of x, dst, residual sits one float behind a 16-byte boundary, or the destination's batch stride is the dense
    size + 2 floats: the scalar kernel, and the bits of the float4 kernel (one expression per element).  Only a caller of the C entry
    point can do this; the Python wrappers take contiguous tensors."""
    shape = (2, 3, 4, 6)
    aligned = check_bias_act(lib, dev, shape, act, mode, mode != 2, "aligned")
    hows = {"x + 4 bytes": dict(x_off=1), "dst + 4 bytes": dict(dst_off=1), "batch stride + 2 floats": dict(stride_extra=2)}
    if mode != 0:
        hows["residual + 4 bytes"] = dict(res_off=1)
    for label, how in hows.items():
        got = check_bias_act(lib, dev, shape, act, mode, False, label, **how)
        assert torch.equal(got, aligned), label


@pytest.mark.parametrize("shape,vec4", [((1, 1, 256, 320), True), ((1, 2, 129, 131), False)])
def test_bias_act_grid_stride_loops(lib, dev, shape, vec4):
    """grid.x = min(ceil(work / 256), 64) with work = HW / 4 (float4) or HW: the loops run above 65 536 and 16 384 pixels per plane --
    the decoder's last layer (1, 1, 256, 320) with the sigmoid -> depth activation, and an odd 129 x 131 plane."""
    assert shape[2] * shape[3] > (4 if vec4 else 1) * 64 * 256
    for act, mode in ((3, 0), (3, 1), (1, 1)):
        check_bias_act(lib, dev, shape, act, mode, vec4, "grid-stride")


@pytest.mark.parametrize("B", [1, 2])
def test_bias_act_wrappers_into_a_channel_slice(ops, lib, dev, B):
    """ops.bias_act_into (channel slice of a [B, 16, H, W] buffer: batch stride 16 * HW) and ops.bias_act_ (in place) give the bits of
    the C entry point; the channels around the slice keep the canary."""
    shape = (B, 7, 6, 10)
    for act, mode in ((0, 0), (1, 1), (2, 2), (3, 1), (3, 2)):
        x, bias, res, p0, p1 = bias_act_problem(shape, act, mode)
        direct, _ = run_bias_act(lib, dev, x, bias, act, res, mode, p0, p1)
        big = torch.full((B, 16, 6, 10), CANARY, device=dev)
        ops.bias_act_into(x.to(dev), big[:, 4:11], bias.to(dev), act, None if res is None else res.to(dev), mode, p0, p1)
        assert torch.equal(big[:, 4:11], direct) and bool((big[:, :4] == CANARY).all()) and bool((big[:, 11:] == CANARY).all())
        ref64 = fr.bias_act(x, bias, act, res, mode, p0, p1, dtype=torch.float64)
        check("bias_act", big[:, 4:11], fr.bias_act(x, bias, act, res, mode, p0, p1), ref64, relative=act == 3, label=f"{shape} slice act={act} res={mode}")
        if act != 3:
            y = x.to(dev).clone()
            ops.bias_act_(y, bias.to(dev), act, torch.empty(0, device=dev) if res is None else res.to(dev), mode)
            assert torch.equal(y, direct)


def test_bias_act_refuses_without_a_launch(lib, dev):
    """B*C = 65 536 (blockIdx.y), odd H or W with the half-resolution residual, a batch stride smaller than C*H*W, and the in-place
    entry with the parametrised activation 3: an error code, and not one float of the destination written."""
    s = _stream(dev)
    x = torch.zeros(65536, device=dev)
    cv = Canvas(dev, 1, 65536)
    calls = {
        "B*C = 65536": (lambda: lib.dvmvs_bias_act_fwd(x.data_ptr(), cv.ptr, 65536, None, None, 0, 1, 65536, 1, 1, 1, 0.0, 0.0, s), EUNSUPPORTED),
        "B*C = 65536 by the batch": (lambda: lib.dvmvs_bias_act_fwd(x.data_ptr(), cv.ptr, 256, None, None, 0, 256, 256, 1, 1, 1, 0.0, 0.0, s), EUNSUPPORTED),
        "odd H, half-resolution residual": (lambda: lib.dvmvs_bias_act_fwd(x.data_ptr(), cv.ptr, 60, None, x.data_ptr(), 2, 2, 2, 5, 6, 0, 0.0, 0.0, s), EUNSUPPORTED),
        "odd W, half-resolution residual": (lambda: lib.dvmvs_bias_act_fwd(x.data_ptr(), cv.ptr, 60, None, x.data_ptr(), 2, 2, 2, 6, 5, 0, 0.0, 0.0, s), EUNSUPPORTED),
        "dst_batch_stride < C*H*W": (lambda: lib.dvmvs_bias_act_fwd(x.data_ptr(), cv.ptr, 71, None, None, 0, 2, 3, 4, 6, 1, 0.0, 0.0, s), EINVAL),
        "residual mode without a residual": (lambda: lib.dvmvs_bias_act_fwd(x.data_ptr(), cv.ptr, 72, None, None, 1, 2, 3, 4, 6, 1, 0.0, 0.0, s), EINVAL),
        "activation 4": (lambda: lib.dvmvs_bias_act_fwd(x.data_ptr(), cv.ptr, 72, None, None, 0, 2, 3, 4, 6, 4, 0.0, 0.0, s), EINVAL),
        "in place with activation 3": (lambda: lib.dvmvs_bias_act_inplace(cv.ptr, None, None, 0, 2, 3, 4, 6, 3, s), EINVAL),
    }
    for what, (call, code) in calls.items():
        assert call() == code, what
        torch.cuda.synchronize(dev)
        assert cv.untouched(), what
    # one below the limit is taken
    assert lib.dvmvs_bias_act_fwd(x.data_ptr(), cv.ptr, 65535, None, None, 0, 1, 65535, 1, 1, 1, 0.0, 0.0, s) == 0
    torch.cuda.synchronize(dev)
    assert cv.outside_intact() and bool((cv.read()[0, :65535] == 0.0).all()) and float(cv.read()[0, 65535]) == CANARY


# ----------------------------------------------------------------------------------------------------------------------
# partial sums + bias + activation: dvmvs_partial_sums_bias_act_fwd (bottleneck_conv.hip)
# ----------------------------------------------------------------------------------------------------------------------
def check_partial_sums(ops, dev, S, shape, bias, act, label):
    B, C, H, W = shape
    parts = _randn((S, B, C, H, W), 71 + S, 10.0)
    b = _randn((C,), 72) if bias else None
    big = torch.full((B, C + 5, H, W), CANARY, device=dev)
    pd, bd = parts.to(dev).reshape(-1), None if b is None else b.to(dev)
    ops.partial_sums_bias_act_into(pd, S, big[:, 3:3 + C], bd, act, shape)
    got = big[:, 3:3 + C].clone()
    assert bool((big[:, :3] == CANARY).all()) and bool((big[:, 3 + C:] == CANARY).all())
    ref32 = fr.partial_sums(parts, b, act)
    check("partial_sums_bias_act", got, ref32, fr.partial_sums(parts, b, act, dtype=torch.float64), label=f"S={S} {shape} bias={bias} act={act} {label}")
    assert torch.equal(got.cpu(), ref32), "the partial sums are the ascending float32 sum, bit for bit"
    dense = torch.full(shape, CANARY, device=dev)
    ops.partial_sums_bias_act_into(pd, S, dense, bd, act, shape)
    assert torch.equal(dense, got), "partial sums: a dense destination / a second launch differs"


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("S", [1, 2, 7, 8, 9, 16, 17, 32])
def test_partial_sums_split_counts(ops, dev, S, bias, act):
    """partial_sums_bias_act_kernel<ACT>: the splits are loaded eight at a time with a guarded tail (``s0 + k < n_partials``) and added in
    ascending order starting FROM split 0 (``s0 + k == 0``), then bias[c] of plane b * C + c, then none | ReLU.  S = 1, 2, 7 stay inside
    the first group, 8, 16, 32 fill their groups, 9 and 17 leave a tail of one; B = 2 into channels [3, 3 + C) of a [B, C + 5] buffer."""
    check_partial_sums(ops, dev, S, (2, 5, 3, 4), bias, act, "channel slice")


def test_partial_sums_grid_stride_loop(ops, dev):
    """grid = min(ceil(B*C*HW / 256), 2048): the loop runs above 2048 * 256 = 524 288 elements per split; (1, 64, 96, 96) has 589 824."""
    shape = (1, 64, 96, 96)
    assert shape[1] * shape[2] * shape[3] > 2048 * 256
    check_partial_sums(ops, dev, 3, shape, True, 1, "grid-stride")


def test_partial_sums_refuses_other_activations(lib, dev):
    parts = torch.zeros(2 * 60, device=dev)
    cv = Canvas(dev, 1, 60)
    assert lib.dvmvs_partial_sums_bias_act_fwd(parts.data_ptr(), 2, cv.ptr, 60, None, 1, 5, 12, 2, _stream(dev)) == EUNSUPPORTED
    assert lib.dvmvs_partial_sums_bias_act_fwd(parts.data_ptr(), 0, cv.ptr, 60, None, 1, 5, 12, 0, _stream(dev)) == EINVAL
    torch.cuda.synchronize(dev)
    assert cv.untouched()

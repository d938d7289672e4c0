"""GPU: every one of the 16 kernels csrc/direct_conv.hip compiles (workgroup shape id 1..4 x kernel size 3, 5 x stride 1, 2) against an
fp64 convolution, on the problems of tests/direct_conv_cases.py -- tests/test_direct_conv_host.py shows without a GPU that they reach all
16 kernels and that every layer of a 320x256 frame at batches 1..8 runs one of them.  Per kernel: a ragged last row tile, a ragged last
input-channel group, a ragged last chunk and whole chunks only; the destination a channel slice of a poisoned concatenation buffer
between canary planes; a repeat; the channels-last second destination.  Then the batch strides of the C entries (direct convolution
and depth head) with NaN in the memory next to every batch item's input, and the strides and pointers the entry has to refuse."""
import pytest
import torch
import torch.nn.functional as F

import direct_conv_cases as dc

pytestmark = pytest.mark.gpu

CANARY = -1234.5
EINVAL = -1


def _ops():
    from dvmvs.hip import ops
    return ops


def _problem(case, seed):
    """x, weight (random, no symmetry), bias on the device and the fp64 convolution without bias, computed once per case."""
    B, C_in, H, W, C_out, k, stride = case
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(seed + C_in * 7 + k * 3 + stride)
    x = torch.randn(B, C_in, H, W, generator=g).to(dev)
    w = (torch.randn(C_out, C_in, k, k, generator=g) / (C_in * k * k) ** 0.5).to(dev)
    bias = torch.randn(C_out, generator=g).to(dev)
    raw = F.conv2d(x.double(), w.double(), None, stride=stride, padding=k // 2)
    return x, w, bias, raw


def _want(raw, bias, act):
    y = raw if bias is None else raw + bias.double()[None, :, None, None]
    return (torch.relu(y) if act else y).float()


def _poisoned_slice(B, C, OH, OW, dev):
    """A [B, 2 + C + 2, OH, OW] concatenation buffer: NaN where the output goes, canary planes in front of and behind it."""
    cat = torch.full((B, C + 4, OH, OW), CANARY, device=dev)
    cat[:, 2:2 + C] = float("nan")
    return cat, cat[:, 2:2 + C]


def _canaries_untouched(cat, C):
    return bool((cat[:, :2] == CANARY).all()) and bool((cat[:, 2 + C:] == CANARY).all())


@pytest.mark.parametrize("case", sorted(dc.CASES), ids=dc.case_id)
def test_variant_matches_fp64_in_a_poisoned_slice(case):
    """The bound is tests/test_direct_conv_gpu.py's: fp32 sums of <= 6 425 terms of O(1/sqrt(n)); the longest sum here has 37 * 25.
    A row written past the last output row of a ragged row tile lands in the next channel's plane: in the canary plane behind the slice
    for the last channel, on another workgroup's values for the others."""
    ops = _ops()
    B, C_in, H, W, C_out, k, stride = case
    variant = dc.CASES[case]
    assert (ops.direct_conv_shape(*case), k, stride) == variant
    n_tile = ops.direct_conv_tile(*case)
    assert n_tile == dc.TILE_OF_SHAPE[variant[0]]
    x, w, bias, raw = _problem(case, 0)
    dev, OH, OW = x.device, H // stride, W // stride
    packed = ops.direct_conv_pack(w, n_tile)
    for act, b in ((1, bias), (0, None)):
        want = _want(raw, b, act)
        cat, dst = _poisoned_slice(B, C_out, OH, OW, dev)
        ops.direct_conv_into(x, packed, n_tile, b, dst, C_out, k, stride, act)
        assert not bool(torch.isnan(dst).any())
        assert _canaries_untouched(cat, C_out)
        err, bound = float((dst - want).abs().max()), 2e-5 * max(1.0, float(want.abs().max()))
        print(f"direct conv kernel (shape {variant[0]}, k {k}, stride {stride}) C_in {C_in} act {act}: max|err| {err:.3e} (bound {bound:.3e})")
        assert err <= bound
        cat2, again = _poisoned_slice(B, C_out, OH, OW, dev)
        ops.direct_conv_into(x, packed, n_tile, b, again, C_out, k, stride, act)
        assert torch.equal(again, dst) and _canaries_untouched(cat2, C_out)
        if C_in == 37:      # the second, channels-last destination: the same bits, and the first destination keeps its own
            cat3, both = _poisoned_slice(B, C_out, OH, OW, dev)
            nhwc = torch.full((B, C_out, OH, OW), float("nan"), device=dev).contiguous(memory_format=torch.channels_last)
            ops.direct_conv_into(x, packed, n_tile, b, both, C_out, k, stride, act, dst_nhwc=nhwc)
            assert torch.equal(both, dst) and _canaries_untouched(cat3, C_out)
            assert torch.equal(nhwc, dst)
            assert torch.equal(nhwc.permute(0, 2, 3, 1).contiguous(), dst.permute(0, 2, 3, 1).contiguous())


@pytest.mark.parametrize("case", sorted(dc.STRIDE_CASES), ids=dc.case_id)
def test_batch_strides_of_the_c_entry_with_nan_next_to_the_input(case):
    """dvmvs_direct_conv_dual_fwd with x_batch_stride > C_in * H * W: every batch item's input is followed by four planes of NaN (and
    the next item).  The kernel requests channels beyond C_in -- the rest of a ragged chunk, the chunk behind the last one -- and relies
    on its `live` predicate and the buffer descriptor's num_records = C_in * H * W to get zeros for them: one NaN read shows in every
    output it reaches.  Same bits as the dense call, in a strided destination as well."""
    from dvmvs.hip import _capi
    from dvmvs.hip.ops._common import launch
    ops = _ops()
    B, C_in, H, W, C_out, k, stride = case
    assert (ops.direct_conv_shape(*case), k, stride) == dc.STRIDE_CASES[case] and B >= 2
    n_tile = ops.direct_conv_tile(*case)
    x, w, bias, raw = _problem(case, 1)
    dev, OH, OW = x.device, H // stride, W // stride
    packed = ops.direct_conv_pack(w, n_tile)
    dense = torch.full((B, C_out, OH, OW), float("nan"), device=dev)
    ops.direct_conv_into(x, packed, n_tile, bias, dense, C_out, k, stride, 1)
    want = _want(raw, bias, 1)
    assert float((dense - want).abs().max()) <= 2e-5 * max(1.0, float(want.abs().max()))

    padded = torch.full((B, C_in + 4, H, W), float("nan"), device=dev)
    padded[:, :C_in] = x
    x_stride = (C_in + 4) * H * W
    assert x_stride % 4 == 0 and padded.data_ptr() % 16 == 0
    cat, dst = _poisoned_slice(B, C_out, OH, OW, dev)
    args = (packed.data_ptr(), n_tile, bias.data_ptr(), dst.data_ptr(), dst.stride(0), None, B, C_in, H, W, C_out, k, stride, 1)
    launch("dvmvs_direct_conv_dual_fwd", dev, padded.data_ptr(), x_stride, *args)
    assert not bool(torch.isnan(dst).any())
    assert torch.equal(dst, dense) and _canaries_untouched(cat, C_out)

    # refused before anything is launched: a batch stride shorter than an item, one that is no multiple of four floats, a pointer off 16 bytes
    cat, dst = _poisoned_slice(B, C_out, OH, OW, dev)
    args = (packed.data_ptr(), n_tile, bias.data_ptr(), dst.data_ptr(), dst.stride(0), None, B, C_in, H, W, C_out, k, stride, 1)
    stream = torch.cuda.current_stream(dev).cuda_stream
    entry = _capi.lib().dvmvs_direct_conv_dual_fwd
    assert entry(padded.data_ptr(), C_in * H * W - 4, *args, stream) == EINVAL
    assert entry(padded.data_ptr(), x_stride + 2, *args, stream) == ops.EUNSUPPORTED
    assert entry(padded.data_ptr() + 4, x_stride, *args, stream) == ops.EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(dst).all()) and _canaries_untouched(cat, C_out)


@pytest.mark.parametrize("size", [(128, 128), (127, 129)], ids=["64-pixel-kernel", "16-pixel-kernel"])
def test_conv_head_batch_strides_with_nan_next_to_the_input(size):
    """dvmvs_conv_head_fwd's two kernels (H * W >= 16 384: 64 pixels x 4 channel slices per workgroup; below: 16 x 16), each batch item's
    input followed by four planes of NaN, the destination one plane of a poisoned three-plane buffer: the dense call's bits, the fp64
    convolution within tests/test_direct_conv_gpu.py's bound, nothing else written."""
    from dvmvs.hip.ops._common import launch
    ops = _ops()
    H, W = size
    B, C = 2, 5
    assert (H * W >= 16384) == (size == (128, 128))
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(H)
    x = torch.randn(B, C, H, W, generator=g).to(dev)
    w = (torch.randn(1, C, 3, 3, generator=g) / (C * 9) ** 0.5).to(dev)
    bias = torch.randn(1, generator=g).to(dev)
    raw = F.conv2d(x.double(), w.double(), padding=1)
    padded = torch.full((B, C + 4, H, W), float("nan"), device=dev)
    padded[:, :C] = x
    for act, b, want, bound in ((0, None, raw, 1e-5), (ops.ACTIVATIONS["sigmoid"], bias, torch.sigmoid(raw + bias.double()), 1e-6)):
        dense = torch.full((B, 1, H, W), float("nan"), device=dev)
        ops.conv_head_into(x, w, b, dense, act)
        assert float((dense - want.float()).abs().max()) <= bound
        cat = torch.full((B, 3, H, W), CANARY, device=dev)
        cat[:, 1] = float("nan")
        dst = cat[:, 1:2]
        launch("dvmvs_conv_head_fwd", dev, padded.data_ptr(), (C + 4) * H * W, w.data_ptr(), None if b is None else b.data_ptr(), dst.data_ptr(),
               3 * H * W, B, C, H, W, int(act), 0.0, 0.0)
        assert not bool(torch.isnan(dst).any())
        assert torch.equal(dst, dense)
        assert bool((cat[:, 0] == CANARY).all()) and bool((cat[:, 2] == CANARY).all())

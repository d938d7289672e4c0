"""The three forward entries of the recurrent chain -- dvmvs_lstm_gates_fwd and dvmvs_lstm_gates_partials_fwd (csrc/lstm_gates.hip) and
dvmvs_hidden_warp_fwd (csrc/hidden_warp.hip) -- on every path their launchers pick from the shape and the number of partial sums.

The arbiter is float64: tests/frame_reference.py states each op once (pinned on the CPU by tests/test_frame_reference.py: the oracle bit
for bit in float32, ATen's LayerNorm / CELU / grid_sample in float64), its float32 call is ``ref32`` and its float64 call ``ref64``, and
every value comparison is ``accuracy.as_accurate_as_reference(got, ref32, ref64)`` with its defaults (slack 3, floor 2e-6) over ALL
elements, the same for every case.  The gates are continuous functions; the warp is continuous except where the source-camera z
crosses the clamp at 0, and every warp case asserts that no pixel's float64 z is within 0.05 of it, so there is no exclusion rule.
Where a kernel promises more, that is asserted too: the gates on partial sums are the gates on the ascending float32 sum bit for bit,
the in-place forms equal the allocating ops bit for bit, and all three kernels are atomics-free: a second launch repeats bit for bit.
Destinations are contiguous views into canary-filled buffers; everything outside the view must keep the canary.

Each section's docstring lists the kernel's paths by the condition in the launcher that selects them, next to the case that takes
each.  Sections print the kernel's and the float32 reference's largest distance to float64 (run with -s to see them).
"""
import math

import pytest
import torch

import frame_reference as fr
import state_cases as sc
from accuracy import as_accurate_as_reference

pytestmark = pytest.mark.gpu

CANARY = -12345.0
PAD = 64                      # floats of canary in front of and behind every destination
NAN = float("nan")

STATS = {}


@pytest.fixture(scope="module")
def dev(hip_device):
    from dvmvs.hip import _capi
    _capi.lib()  # the HIP library must be there: no fallback
    yield hip_device
    for section, (ek, er, n) in STATS.items():
        print(f"\n[state kernels] {section}: {n} comparisons, max |kernel - float64| {ek:.2e} (float32 reference: {er:.2e})")


@pytest.fixture(scope="module")
def ops(dev):
    from dvmvs.hip import ops as o
    return o


def _randn(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def check(section, got, ref32, ref64, label=""):
    """The one value comparison of this module."""
    got = got.detach().cpu()
    assert got.shape == ref64.shape and ref64.dtype == torch.float64 and ref32.dtype == torch.float32, label
    assert torch.isfinite(got).all(), label
    g, r32 = got.double(), ref32.double()
    ek, er = float((g - ref64).abs().max()), float((r32 - ref64).abs().max())
    s = STATS.setdefault(section, [0.0, 0.0, 0])
    s[0], s[1], s[2] = max(s[0], ek), max(s[1], er), s[2] + 1
    print(f"{section} {label}: max |kernel - float64| {ek:.2e} (float32 reference: {er:.2e})")
    as_accurate_as_reference(g, r32, ref64)


def carve(dev, shape):
    """A canary-filled buffer and the contiguous view of ``shape`` in its middle, PAD canaries on either side."""
    n = math.prod(shape)
    buf = torch.full((n + 2 * PAD,), CANARY, device=dev)
    return buf, buf[PAD:PAD + n].view(shape)


def intact(buf):
    return bool((buf[:PAD] == CANARY).all()) and bool((buf[-PAD:] == CANARY).all())


def nan_rows(t):
    """[B, C] mask of the (batch, channel) planes that are NaN everywhere; asserts that no plane is NaN only in part."""
    bad = torch.isnan(t.detach().cpu()).flatten(2)
    assert bool((bad.all(dim=2) == bad.any(dim=2)).all()), "a plane is NaN in part"
    return bad.all(dim=2)


def only_row(B, C, b, ch):
    m = torch.zeros(B, C, dtype=torch.bool)
    m[b, ch] = True
    return m


# ----------------------------------------------------------------------------------------------------------------------
# gates forward: dvmvs_lstm_gates_fwd
# ----------------------------------------------------------------------------------------------------------------------
def run_gates(ops, dev, cc, c):
    """(h', c') of ``ops.lstm_gates_into`` -- c' written over c -- with both states carved out of canary buffers, launched twice, and
    equal bit for bit to the allocating ``ops.lstm_gates`` (separate c')."""
    ccd, outs = cc.to(dev), []
    for _ in range(2):
        (cbuf, cst), (hbuf, hst) = carve(dev, c.shape), carve(dev, c.shape)
        cst.copy_(c)
        ops.lstm_gates_into(ccd, cst, hst)
        torch.cuda.synchronize(dev)
        assert intact(cbuf) and intact(hbuf), tuple(c.shape)
        outs.append((hst.clone(), cst.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "the gates are not bit-reproducible"
    h, cn = ops.lstm_gates(ccd, c.to(dev))
    assert torch.equal(h, outs[0][0]) and torch.equal(cn, outs[0][1]), "lstm_gates_into (c aliases c') differs from lstm_gates"
    return outs[0]


def check_gates(ops, dev, cc, c, label):
    h, cn = run_gates(ops, dev, cc, c)
    (h32, c32), (h64, c64) = fr.lstm_gates(cc, c), fr.lstm_gates(cc, c, dtype=torch.float64)
    check("lstm_gates_fwd", h, h32, h64, label + " h'")
    check("lstm_gates_fwd", cn, c32, c64, label + " c'")


GATE_LAYOUTS = {(1, 1): (16, 4), (1, 5): (16, 4), (3, 5): (16, 4), (8, 8): (16, 4), (5, 13): (64, 2), (8, 10): (64, 2), (8, 16): (64, 2),
                (3, 43): (64, 4), (16, 16): (64, 4), (1, 257): (64, 8), (16, 32): (64, 8), (19, 27): (64, 16), (32, 32): (64, 16)}


@pytest.mark.parametrize("H,W", sc.GATE_MAPS)
def test_gates_forward_every_layout(ops, dev, H, W):
    """dispatch_gates<true> picks lstm_gates_fwd_kernel<lanes per row, elements per lane> from H*W:
    * ``HW <= 16*4``  <16,4>:  (1,1) = 1, (1,5) = 5, (3,5) = 15, (8,8) = 64 (the boundary);
    * ``HW <= 64*2``  <64,2>:  (5,13) = 65, (8,10) = 80 (the frame's cell), (8,16) = 128;
    * ``HW <= 64*4``  <64,4>:  (3,43) = 129, (16,16) = 256;
    * ``HW <= 64*8``  <64,8>:  (1,257) = 257, (16,32) = 512;
    * ``HW <= 64*16`` <64,16>: (19,27) = 513, (32,32) = 1024;
    * larger planes are refused (test_gates_refuse_planes_above_1024_elements).
    B = 3, hid = 5: 15 rows leave the last workgroup partly empty in every layout (16 rows per workgroup in <16,4>, 4 in the others)."""
    assert sc.gate_layout(H * W) == GATE_LAYOUTS[(H, W)]
    cc, c = sc.gate_inputs(3, 5, H, W, seed=100 + H * W)
    check_gates(ops, dev, cc, c, f"{H}x{W}")


@pytest.mark.parametrize("H,W", [(8, 8), (8, 10), (16, 16), (16, 32), (32, 32)])
def test_gates_forward_full_workgroups(ops, dev, H, W):
    """One case per layout whose 16 rows (B = 1, hid = 16) fill their workgroups: one of <16,4>, four of the one-wave-per-row layouts."""
    cc, c = sc.gate_inputs(1, 16, H, W, seed=200 + H * W)
    check_gates(ops, dev, cc, c, f"{H}x{W} full workgroups")


@pytest.mark.parametrize("kind", ["narrow", "saturated"])
@pytest.mark.parametrize("H,W", [(8, 8), (8, 10), (16, 16), (16, 32), (19, 27)])
def test_gates_forward_hard_values(ops, dev, H, W, kind):
    """The hard values of the backward suite, once per layout: ``narrow`` g rows of offset 5 and sigma 1e-3 (the LayerNorm amplifies
    the float32 round-off of the mean by 1000 -- in the reference just as in the kernel, which is what the criterion measures), and
    ``saturated`` |cc| around 20 with single outliers in two g rows and one cell-state row."""
    cc, c = sc.hard_gate_inputs(kind, 3, 5, H, W, seed=400 + H * W)
    check_gates(ops, dev, cc, c, f"{H}x{W} {kind}")


@pytest.mark.parametrize("H,W", sc.GATE_MAPS)
def test_gates_rows_are_isolated(ops, dev, H, W):
    """A NaN in one element of one (batch, channel) row of cc -- in each of the four gates in turn -- or of c makes exactly that row of
    h' and c' NaN (the row's LayerNorm spreads it) and leaves every other element with the bits of the clean run, in every layout:
    rows share a wavefront (four rows in <16,4>) and a workgroup, never a sum."""
    B, hid = 3, 5
    cc, c = sc.gate_inputs(B, hid, H, W, seed=100 + H * W)
    clean_h, clean_c = ops.lstm_gates(cc.to(dev), c.to(dev))
    e = (H * W) // 2
    for what in ("i", "f", "o", "g", "c"):
        b, ch = ("ifogc".index(what) + 1) % B, ("ifogc".index(what) * 2 + 1) % hid
        cc_bad, c_bad = cc.clone(), c.clone()
        if what == "c":
            c_bad[b, ch].view(-1)[e] = NAN
        else:
            cc_bad[b, "ifog".index(what) * hid + ch].view(-1)[e] = NAN
        h, cn = ops.lstm_gates(cc_bad.to(dev), c_bad.to(dev))
        want = only_row(B, hid, b, ch)
        # (the o gate enters h' only, element by element: c' stays clean and h' is NaN in that one element)
        if what == "o":
            assert not bool(torch.isnan(cn).any()) and torch.equal(cn, clean_c)
            bad = torch.isnan(h.cpu())
            assert int(bad.sum()) == 1 and bool(bad[b, ch].view(-1)[e])
        else:
            assert torch.equal(nan_rows(h), want) and torch.equal(nan_rows(cn), want), what
        keep = ~torch.isnan(h)
        assert torch.equal(h[keep], clean_h[keep]) and torch.equal(cn[~torch.isnan(cn)], clean_c[~torch.isnan(cn)]), what


def test_gates_refuse_planes_above_1024_elements(ops, dev):
    """``HW > 64*16``: 25 x 41 = 1025, one above the last layout, is refused by every entry and the destinations keep their contents."""
    B, hid, H, W = 2, 3, 25, 41
    assert sc.gate_layout(H * W) is None and sc.gate_layout(H * W - 1) == (64, 16)
    cc, c = sc.gate_inputs(B, hid, H, W, seed=1025)
    with pytest.raises(RuntimeError, match="dvmvs_lstm_gates_fwd"):
        ops.lstm_gates(cc.to(dev), c.to(dev))
    (cbuf, cst), (hbuf, hst) = carve(dev, c.shape), carve(dev, c.shape)
    with pytest.raises(RuntimeError, match="dvmvs_lstm_gates_fwd"):
        ops.lstm_gates_into(cc.to(dev), cst, hst)
    with pytest.raises(RuntimeError, match="dvmvs_lstm_gates_partials_fwd"):
        ops.lstm_gates_partials_into(torch.stack([cc, cc]).to(dev), 2, cst, hst)
    torch.cuda.synchronize(dev)
    assert bool((cbuf == CANARY).all()) and bool((hbuf == CANARY).all())


# ----------------------------------------------------------------------------------------------------------------------
# gates on partial sums: dvmvs_lstm_gates_partials_fwd
# ----------------------------------------------------------------------------------------------------------------------
PARTIAL_MAPS = {64: (8, 8), 65: (5, 13), 80: (8, 10), 128: (8, 16), 129: (3, 43), 320: (16, 20), 513: (19, 27)}
PARTIAL_SPLITS = [1, 2, 5, 6, 16]
TAIL = 1024                   # floats of NaN behind the partial sums


def run_partials(ops, dev, flat, S, c):
    outs = []
    for _ in range(2):
        (cbuf, cst), (hbuf, hst) = carve(dev, c.shape), carve(dev, c.shape)
        cst.copy_(c)
        ops.lstm_gates_partials_into(flat, S, cst, hst)
        torch.cuda.synchronize(dev)
        assert intact(cbuf) and intact(hbuf)
        outs.append((hst.clone(), cst.clone()))
    return outs


def with_nan_tail(dev, parts):
    """The partial sums in a buffer that is TAIL floats longer than S*B*4*hid*H*W, the tail filled with NaN."""
    flat = torch.full((parts.numel() + TAIL,), NAN, device=dev)
    flat[:parts.numel()] = parts.reshape(-1).to(dev)
    return flat


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("HW", sorted(PARTIAL_MAPS))
def test_gates_on_partial_sums(ops, dev, HW, B):
    """Paths of dvmvs_lstm_gates_partials_fwd -- the WHOLE product H*W x S x B is run (7 x 5 x 2 = 70 cases of hid = 5, i.e. 5 or 10
    rows: a partly empty workgroup in every dispatch_gates layout):
    * ``n_partials > 1 && HW > 64 && HW <= 128``: lstm_gates_partials_kernel, four waves per row (wave w sums gate w, the sums meet in
      LDS) -- H*W = 65 (lane 0 alone owns a second element), 80, 128 (every lane does) with S = 2, 5, 6, 16;
    * otherwise dispatch_gates with the partial-sum loop: H*W = 64 -> <16,4> (one below the four-wave kernel), 129 -> <64,4> (one
      above it), 320 -> <64,8>, 513 -> <64,16>, and S = 1 at 65, 80, 128 -> <64,2> (the loop body never runs).
    The loops run s = 1 .. S-1 under ``#pragma unroll 4``: S = 1 no trip, S = 2 one trip (remainder only), S = 5 four (one unrolled
    body, no remainder), S = 6 five (a body and a remainder of one), S = 16 fifteen (three bodies and a remainder of three).
    B = 2 makes the partial stride B*4*hid*HW differ from one item's 4*hid*HW.
    Per case: bit-equal to lstm_gates_into on the ascending float32 sum (and so, at S = 1, to lstm_gates on the one part); as accurate
    as the float32 reference against float64; a NaN in one split of one row reaches exactly that row; nothing of the NaN tail behind
    the S*B*4*hid*HW partial sums reaches an output."""
    H, W = PARTIAL_MAPS[HW]
    hid = 5
    for S in PARTIAL_SPLITS:
        four_waves = S > 1 and 64 < HW <= 128
        parts, c = _randn((S, B, 4 * hid, H, W), 500 + HW + S, 1.5 / S ** 0.5), _randn((B, hid, H, W), 501 + HW)
        label = f"HW={HW} S={S} B={B} ({'four waves per row' if four_waves else 'dispatch_gates %s' % (sc.gate_layout(HW),)})"
        first, again = run_partials(ops, dev, with_nan_tail(dev, parts), S, c)
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1]), "the gates on partial sums are not bit-reproducible"
        total = fr.partial_sums(parts)                                  # ascending float32 sum: IEEE additions, the same on any device
        h_sum, c_sum = run_gates(ops, dev, total, c)
        assert torch.equal(first[0], h_sum) and torch.equal(first[1], c_sum), label
        (h32, c32), (h64, c64) = fr.lstm_gates_partials(parts, c), fr.lstm_gates_partials(parts, c, dtype=torch.float64)
        check("lstm_gates_partials_fwd", first[0], h32, h64, label + " h'")
        check("lstm_gates_partials_fwd", first[1], c32, c64, label + " c'")
        # one NaN in one split (the last, which only the loop reads; split 0 at S = 1) of one row, in gate S % 4 but never o (see above)
        b, ch, gate = B - 1, S % hid, (0, 1, 3)[S % 3]
        bad = parts.clone()
        bad[S - 1, b, gate * hid + ch].view(-1)[HW - 1] = NAN
        h_bad, c_bad = run_partials(ops, dev, with_nan_tail(dev, bad), S, c)[0]
        want = only_row(B, hid, b, ch)
        assert torch.equal(nan_rows(h_bad), want) and torch.equal(nan_rows(c_bad), want), label
        keep = ~torch.isnan(h_bad)
        assert torch.equal(h_bad[keep], first[0][keep]) and torch.equal(c_bad[keep], first[1][keep]), label


# ----------------------------------------------------------------------------------------------------------------------
# hidden-state warp forward: dvmvs_hidden_warp_fwd
# ----------------------------------------------------------------------------------------------------------------------
def run_warp(ops, dev, src, depth, T, K, mask):
    """``ops.hidden_warp_into`` into a view carved out of a canary buffer, twice, and equal to the allocating ``ops.hidden_warp``."""
    sd, dd, Td, Kd = (t.to(dev) for t in (src, depth, T, K))
    outs = []
    for _ in range(2):
        buf, dst = carve(dev, src.shape)
        ops.hidden_warp_into(sd, dd, Td, Kd, mask, dst)
        torch.cuda.synchronize(dev)
        assert intact(buf)
        outs.append(dst.clone())
    assert torch.equal(outs[0], outs[1]), "the hidden-state warp is not bit-reproducible"
    assert torch.equal(ops.hidden_warp(sd, dd, Td, Kd, mask), outs[0]), "hidden_warp_into differs from hidden_warp"
    return outs[0]


def check_warp(ops, dev, shape, kind):
    B, C, H, W = shape
    depth, T, K = sc.warp_case(kind, B, H, W, seed=900 + H * W)
    src = _randn(shape, 901 + C)
    gone = (depth <= torch.tensor(0.01, dtype=torch.float32)).expand(B, C, H, W)
    for mask in (False, True):
        ref32, ix, iy, z = fr.hidden_warp(src, depth, T, K, mask)
        ref64 = fr.hidden_warp(src, depth, T, K, mask, dtype=torch.float64)[0]
        counts = sc.check_warp_case(kind, depth, ix, iy, z, H, W)      # the class is there and no |z| <= 0.05: proven from float64
        got = run_warp(ops, dev, src, depth, T, K, mask)
        check("hidden_warp_fwd", got, ref32, ref64, f"{shape} {kind} zero_invalid={mask} {counts}")
        if mask:
            assert float(got.cpu()[gone].abs().max() if gone.any() else 0.0) == 0.0
    return counts


@pytest.mark.parametrize("kind", sc.WARP_KINDS)
@pytest.mark.parametrize("shape", sc.WARP_SHAPES)
def test_hidden_warp_forward(ops, dev, shape, kind):
    """hidden_warp_fwd_kernel, one thread per output element (``total <= 2048 * 256``: every shape here), on geometries built by
    construction (tests/state_cases.py) with a different transform and camera matrix per batch item; per kind, proven in the test from
    the float64 reference's sample positions and source-camera z:
    * ``sideways``  small sideways motion; depths hold 0, 0.01f, the next float above it and positive values; the points of depth 0
                    land at the translation itself: pixels with ALL FOUR TAPS OUTSIDE, next to pixels inside;
    * ``shift``     pure in-plane shift at constant depth: every sample at (x + sx, y + sy), a fractional number of pixels;
    * ``forward``   strong forward motion: every sample inside the map (the special depths too);
    * ``behind``    every point behind the source camera: ``relu`` clamps z to 0 and ``|z| > eps ? 1/z : 1`` takes its second
                    branch for EVERY pixel;
    * ``borders``   magnified about the principal point so that the north-west tap sits in column -1, in column W-1, in row -1 and in
                    row H-1 for some pixels each (where the map has more than one column / row).
    Precondition per case: every pixel's float64 z before the clamp is below -0.05 or above 0.05.  H == 1 and W == 1 normalise by
    max(size - 1, 1e-8): the sample's row / column is 0 whatever the geometry.  Both ``zero_invalid`` settings; the mask takes 0 and
    0.01f and leaves the next float above."""
    check_warp(ops, dev, shape, kind)


@pytest.mark.parametrize("kind", ["sideways", "behind"])
def test_hidden_warp_forward_grid_stride_loop(ops, dev, kind):
    """``total > 2048 * 256``: the grid is capped at 2048 workgroups and the loop runs -- (2, 1100, 15, 16) has 528 000 elements, so
    3712 threads take a second element (of batch item 1)."""
    B, C, H, W = sc.WARP_GRID_STRIDE_SHAPE
    assert 2048 * 256 < B * C * H * W < 2 * 2048 * 256
    check_warp(ops, dev, sc.WARP_GRID_STRIDE_SHAPE, kind)


def test_hidden_warp_classes_are_all_present():
    """Across the cases above: a north-west tap at x = -1, at x = W-1, at y = -1, at y = H-1, all four taps outside, z clamped."""
    seen = dict(west=0, east=0, north=0, south=0, outside=0, clamped=0)
    for B, C, H, W in sc.WARP_SHAPES[:2]:         # the two shapes with more than one row and column and more than one batch item
        for kind in sc.WARP_KINDS:
            depth, T, K = sc.warp_case(kind, B, H, W, seed=900 + H * W)
            grid, z = fr.warp_grid(depth, T, K, torch.float64)
            n = sc.warp_classes(fr.grid_pixels(grid[..., 0], W), fr.grid_pixels(grid[..., 1], H), z, H, W)
            for k in seen:
                seen[k] += n[k]
    assert all(v > 0 for v in seen.values()), seen


def test_hidden_warp_into_the_upper_channel_half(ops, dev):
    """What the frame engine does: the warped state goes into channels [512, 1024) of the cell's [1, 1024, 8, 10] input buffer (a
    contiguous view at B = 1); the lower half keeps its contents."""
    B, C, H, W = 1, 512, 8, 10
    depth, T, K = sc.warp_case("sideways", B, H, W, seed=900 + H * W)
    src = _randn((B, C, H, W), 901 + C)
    args = [t.to(dev) for t in (src, depth, T, K)]
    big = torch.full((B, 2 * C, H, W), CANARY, device=dev)
    assert ops.hidden_warp_into(*args, True, big[:, C:]).data_ptr() == big[:, C:].data_ptr()
    torch.cuda.synchronize(dev)
    assert torch.equal(big[:, C:], ops.hidden_warp(*args, True)) and bool((big[:, :C] == CANARY).all())


def test_hidden_warp_refuses_mismatched_shapes_without_a_launch(ops, dev):
    """depth, transform and intrinsics of batch 1 for a source of batch 2 (the kernel would read past their ends), and a depth of
    another map size: ValueError from ``ops.hidden_warp``, ``ops.hidden_warp_into`` and ``utils.warp_frame_depth``, and not one float
    of the destination written."""
    from dvmvs import utils
    B, C, H, W = 2, 3, 4, 5
    depth, T, K = sc.warp_case("sideways", B, H, W, seed=1)
    good = [t.to(dev) for t in (_randn((B, C, H, W), 2), depth, T, K)]
    buf, dst = carve(dev, (B, C, H, W))
    wrong = {"depth_dst": (1, [good[1][:1], good[1][:, :, :, :4].contiguous()]), "src_trans_dst": (2, [good[2][:1]]), "camera_matrix": (3, [good[3][:1]])}
    for name, (pos, tensors) in wrong.items():
        for t in tensors:
            args = list(good)
            args[pos] = t
            with pytest.raises(ValueError, match=name):
                ops.hidden_warp(*args, True)
            with pytest.raises(ValueError, match=name):
                ops.hidden_warp_into(*args, True, dst)
            with pytest.raises(ValueError, match=name):
                utils.warp_frame_depth(*args)
    with pytest.raises(ValueError, match="dst"):
        ops.hidden_warp_into(*good, True, dst[:1])
    torch.cuda.synchronize(dev)
    assert bool((buf == CANARY).all())
    ops.hidden_warp_into(*good, True, dst)                 # the well-formed call is taken
    torch.cuda.synchronize(dev)
    assert intact(buf) and torch.equal(dst, ops.hidden_warp(*good, True))
    assert torch.equal(utils.warp_frame_depth(*good), ops.hidden_warp(*good, False))

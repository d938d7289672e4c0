"""The LDS-tiled plane sweep (csrc/sweep_tiled.hip, variants 2 / 3 / 4 / 5 of dvmvs_cost_volume_planned_fwd) launched FROM A WORK LIST -- what
DepthEngine launches for every lock-step batch, for every frame of an engine built with DVMVS_SWEEP_MFMA=0 and for maps below 64 x 64 cells.  A
workgroup then takes an item {tile | batch << 16, first plane | planes << 16} instead of a static (tile, chunk of 8 planes) pair; long pairs are cut
into plane sub-ranges, the extra pieces sit behind the static positions, padding positions have 0 planes, the spill slot of the second pass is indexed
by the item number and the second pass reads the item's plane range.

Checked here, with a list present, against the CPU oracle in float32 and float64 (tests/accuracy.py: the kernel may be 3 x as far from float64 as the
float32 oracle is, floors 2e-6 / 1e-5 for channels-last maps as in tests/test_hip_parity.py): the host planner's own lists on easy, wide-baseline and
forward-motion keyframe pairs (all four variants come back), ragged and tiny shapes, one and two channel passes; lists the planner did not make for
the geometry (every pair halved, another geometry's list, an uncut list on a geometry that needs the inline gather); batches; the spill workspace
after list launches; refusals.  Every launch writes into a NaN-filled destination: "every item's planes are written exactly once".

The plans themselves (variant, items against static positions) are asserted without a GPU in tests/test_sweep_plan.py.
Semantics under test: the reference's cost_volume_fusion (dvmvs/utils.py:45-107)."""
import functools
from collections import namedtuple

import pytest
import torch

import dvmvs_oracle as orc
import sweep_lists as sl
import synthetic as syn
from accuracy import as_accurate_as_reference, f64

pytestmark = pytest.mark.gpu

Inputs = namedtuple("Inputs", "shape f1 f2s p1 p2s K Hm kt")
FEATURE_SET = {170: 1, 202: 2}      # full shape: which of three feature sets a line reads (so that a batch of lines 0 / 170 / 202 has its own maps per item)


@pytest.fixture(scope="module")
def ops(hip_device):
    from dvmvs.hip import _capi, ops as o
    _capi.lib()      # the HIP library must be there: no fallback
    return o


@functools.lru_cache(maxsize=None)
def feature_maps(shape):
    """(reference map, measurement maps) on the host: smooth noise at the full shape (three sets), seeded white noise at the others."""
    B, C, H, W, D, M = shape
    if shape == sl.FULL[0]:
        return tuple(syn.smooth_noise((3, C, H, W), seed=1700 + i) for i in range(M + 1))
    g = torch.Generator().manual_seed(B * 1000 + C * 100 + H)
    return tuple(torch.randn(B, C, H, W, generator=g) for _ in range(M + 1))


@functools.lru_cache(maxsize=None)
def inputs(case, lines):
    """Host inputs of `lines` (one batch item per keyframe index line) at a case's shape."""
    shape, k_scale = case
    maps = feature_maps(shape)
    if shape == sl.FULL[0]:
        maps = [torch.cat([t[FEATURE_SET.get(line, 0)][None] for line in lines]) for t in maps]
    p1, p2s = sl.poses(lines)
    Hm, kt = sl.matrices(lines, k_scale)
    return Inputs((len(lines),) + shape[1:], maps[0], list(maps[1:]), p1, p2s, sl.intrinsics(lines, k_scale), Hm, kt)


@functools.lru_cache(maxsize=None)
def reference(case, line):
    """(float32 oracle, float64 oracle) of one line: evaluated once, shared by every test, never modified."""
    i = inputs(case, (line,))
    D = i.shape[4]
    return (orc.cost_volume_fusion(i.f1, i.f2s, i.p1, i.p2s, i.K, sl.LO, sl.HI, D, True),
            orc.cost_volume_fusion(*f64(i.f1, i.f2s, i.p1, i.p2s, i.K), sl.LO, sl.HI, D, True))


def layouts(shape):
    B, C, H, W, D, M = shape
    return (False, True) if H * W >= 64 * 64 and C % 4 == 0 and shape != sl.ONE_PASS_12[0] else (False,)      # (12 channels: a ragged second pass, NCHW)


def on_device(dev, i, nhwc):
    f2s = [t.to(dev) for t in i.f2s]
    if nhwc:
        f2s = [t.contiguous(memory_format=torch.channels_last) for t in f2s]
        assert all(not t.is_contiguous() for t in f2s)
    return i.f1.to(dev), f2s, i.Hm.to(dev), i.kt.to(dev)


def launch_into(ops, dev, i, variant, words, nhwc=False):
    """ops.cost_volume_into on a NaN-filled destination."""
    B, C, H, W, D, M = i.shape
    f1, f2s, Hm, kt = on_device(dev, i, nhwc)
    dst = torch.full((B, D, H, W), float("nan"), device=dev)
    ops.cost_volume_into(f1, f2s, Hm, kt, sl.LO, sl.HI, dst, variant, work_list=None if words is None else words.to(dev))
    return dst


def launch_op(ops, dev, i, variant, words, nhwc=False):
    """The registered op (ops.cost_volume): allocates its own result."""
    f1, f2s, Hm, kt = on_device(dev, i, nhwc)
    return ops.cost_volume(f1, f2s, Hm, kt, sl.LO, sl.HI, i.shape[4], True, variant, work_list=None if words is None else words.to(dev))


def written_and_accurate(tag, got, ref, nhwc):
    exp, exp64 = ref
    assert not torch.isnan(got).any(), (tag, "planes nobody wrote")
    g, e, e64 = got.cpu().double(), exp.double(), exp64
    print(f"{tag}{' channels-last' if nhwc else ''}: kernel vs float64 max {float((g - e64).abs().max()):.3e} mean {float((g - e64).abs().mean()):.3e}; "
          f"float32 oracle vs float64 max {float((e - e64).abs().max()):.3e} mean {float((e - e64).abs().mean()):.3e}")
    as_accurate_as_reference(got, exp, exp64, floor=1e-5 if nhwc else 2e-6)


def twice(ops, dev, i, variant, words, nhwc):
    """Both entry points on the same launch: NaN-filled destination first, the registered op second; bit for bit the same volume."""
    first = launch_into(ops, dev, i, variant, words, nhwc)
    second = launch_op(ops, dev, i, variant, words, nhwc)
    assert torch.equal(first, second), "a second launch gives other bits"
    return first


def own_plan(case, line, forced):
    shape, _ = case
    i = inputs(case, (line,))
    variant, words = sl.planned(i.Hm, i.kt, shape[2], shape[3], shape[4], forced)
    return variant, words


# ----------------------------------------------------------------------------------------------------------------------
# 1 + 2: the geometry's own list
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sl.PLAN_CASES))
def test_parity_with_the_geometrys_own_list(ops, hip_device, name):
    """The variant and the list dvmvs_sweep_plan returns for the geometry: every output element written, as close to float64 as the float32 oracle,
    bit-reproducible; at the full shape within 1e-6 of the same variant WITHOUT a list (the bound test_cost_volume_two_pass_is_bit_reproducible holds
    between two forms of this kernel; a cut can change which frame's run is queued, so bit-equality is not claimed).  Host side of the same launch: the
    cases that are here for their cuts do have more items than static positions and items that start off a multiple of 8."""
    case, line, forced, cuts = sl.PLAN_CASES[name]
    shape = case[0]
    variant, words = own_plan(case, line, forced)
    n, items = sl.parse(words)
    static = sl.static_positions(shape[0], shape[2], shape[3], shape[4])
    assert variant in (2, 3, 4, 5) and (forced == 0 or variant == forced)
    assert (sl.coverage(items, shape[0], shape[2], shape[3], shape[4]) == 1).all()
    if cuts:
        assert n > static and ((items[:, 1] & 0xffff) % 8 != 0).any(), (name, n, static)
    else:
        assert n == static
    print(f"{name}: variant {variant}, {n} items against {static} static positions, {int(((items[:, 1] >> 16) == 0).sum())} of them without planes")
    i = inputs(case, (line,))
    for nhwc in layouts(shape):
        got = twice(ops, hip_device, i, variant, words, nhwc)
        written_and_accurate(name, got, reference(case, line), nhwc)
        if case == sl.FULL:
            without = launch_into(ops, hip_device, i, variant, None, nhwc)
            assert float((got - without).abs().max()) < 1e-6, (name, nhwc)


def test_the_full_case_returns_every_tiled_variant():
    """(host only, here so that the GPU run shows it next to what it launched) two-pass and single-pass forms of both configurations."""
    assert {own_plan(case, line, forced)[0] for case, line, forced, _ in sl.PLAN_CASES.values() if case == sl.FULL} == {2, 3, 4, 5}


# ----------------------------------------------------------------------------------------------------------------------
# 3: any partition of (tile, plane) gives the volume
# ----------------------------------------------------------------------------------------------------------------------
FOREIGN = {
    # every (tile, chunk) halved, whatever the geometry needs: all four variants
    "halved-full-0": (sl.FULL, 0, "halved", (2, 3, 4, 5)), "halved-full-141": (sl.FULL, 141, "halved", (2, 3, 4, 5)),
    "halved-full-170": (sl.FULL, 170, "halved", (2, 3, 4, 5)), "halved-ragged-170": (sl.RAGGED, 170, "halved", (2, 3, 4, 5)),
    # the list planned for line 170 (forced 2: 2-plane pieces, items off multiples of 8) on two easy geometries
    "line-170-list-on-full-0": (sl.FULL, 0, 170, (2, 3)), "line-170-list-on-full-141": (sl.FULL, 141, 170, (2, 3)),
    # the uncut list of line 0, for which the host says "nothing queued", as single-pass launches where runs cannot be staged: gathered inline
    "line-0-list-on-full-170": (sl.FULL, 170, 0, (4, 5)), "line-0-list-on-full-202": (sl.FULL, 202, 0, (4, 5)),
}


@pytest.mark.parametrize("name", list(FOREIGN))
def test_any_partition_gives_the_volume(ops, hip_device, name):
    """The kernel plans its runs itself, per item: a list that partitions (tile, plane) gives the volume whoever made it and whatever the host's plan of
    THIS geometry would have been -- no NaN left, float64 criterion, bit-reproducible."""
    case, line, source, variants = FOREIGN[name]
    B, C, H, W, D, M = case[0]
    if source == "halved":
        words = sl.halved(B, H, W, D)
    else:
        planned_as, words = own_plan(case, source, 2 if source == 170 else 0)
        assert planned_as == (2 if source == 170 else 4)
    n, items = sl.parse(words)
    assert (sl.coverage(items, B, H, W, D) == 1).all()
    i = inputs(case, (line,))
    for variant in variants:
        for nhwc in layouts(case[0]):
            got = twice(ops, hip_device, i, variant, words, nhwc)
            written_and_accurate(f"{name} variant {variant}", got, reference(case, line), nhwc)


# ----------------------------------------------------------------------------------------------------------------------
# 4: the batch field
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forced", [0, 2])
def test_batch_items_equal_their_single_launches(ops, hip_device, forced):
    """B = 3 (lines 0, 170, 202; own maps and matrices per item) from one list whose items carry the batch item in bits 16 and up.  The host plans per
    (batch, tile, chunk) and a workgroup adds its contributions in run order, the second pass in queue order, so the arithmetic of an item does not
    depend on its batch: every item equals, BIT FOR BIT, the B = 1 launch of the same variant with that item's own list -- and meets the float64
    criterion, in both layouts."""
    lines = (0, 170, 202)
    B, C, H, W, D, M = sl.FULL[0]
    batch = inputs(sl.FULL, lines)
    variant, words = sl.planned(batch.Hm, batch.kt, H, W, D, forced)
    n, items = sl.parse(words)
    assert variant == (2 if forced else 3)
    assert (sl.coverage(items, 3, H, W, D) == 1).all() and set((items[:, 0] >> 16).tolist()) == {0, 1, 2}
    singles = [own_plan(sl.FULL, line, variant)[1] for line in lines]      # (the batch's configuration, forced)
    assert n == sum(sl.parse(w)[0] for w in singles) > sl.static_positions(3, H, W, D)
    print(f"batch of lines {lines}, forced {forced}: variant {variant}, {n} items against {sl.static_positions(3, H, W, D)} static positions")
    for nhwc in (False, True):
        got = twice(ops, hip_device, batch, variant, words, nhwc)
        for b, line in enumerate(lines):
            one = launch_into(ops, hip_device, inputs(sl.FULL, (line,)), variant, singles[b], nhwc)
            assert torch.equal(got[b], one[0]), (forced, nhwc, line)
            written_and_accurate(f"batch item {b} (line {line}) variant {variant}", got[b:b + 1], reference(sl.FULL, line), nhwc)


# ----------------------------------------------------------------------------------------------------------------------
# 5: the shared spill workspace, channel slices
# ----------------------------------------------------------------------------------------------------------------------
def test_workspace_header_is_restored_after_list_launches(ops, hip_device):
    """The shared workspace (ops.sweep_workspace) between launches: a list-less launch, a list launch that queues runs, a list launch that queues
    nothing, the list-less launch again -- the same bits as the first time, and words 0 / 1 of the header zero after every launch."""
    dev = hip_device
    B, C, H, W, D, M = sl.FULL[0]
    busy, easy = inputs(sl.FULL, (170,)), inputs(sl.FULL, (0,))
    workspace, _ = ops.sweep_workspace(dev, B, M, H, W, D)

    def header():
        return workspace[:2].view(torch.int32).tolist()

    kept = launch_op(ops, dev, busy, 2, None)
    assert header() == [0, 0]
    variant, words = own_plan(sl.FULL, 170, 2)
    assert variant == 2      # (runs queued for the second pass)
    with_list = launch_op(ops, dev, busy, variant, words)
    assert header() == [0, 0]
    variant0, words0 = own_plan(sl.FULL, 0, 0)
    assert variant0 == 4     # (nothing queued) -- launched in its two-pass form, so that the empty second pass runs on the workspace
    launch_op(ops, dev, easy, 2, words0)
    assert header() == [0, 0]
    again = launch_op(ops, dev, busy, 2, None)
    assert header() == [0, 0]
    assert torch.equal(again, kept)
    assert float((with_list - kept).abs().max()) < 1e-6


def test_list_launch_into_a_channel_slice_writes_only_the_slice(ops, hip_device):
    """ops.cost_volume_into with a list into channels [3, 67) of a 70-channel buffer (the engine's encoder input is such a slice)."""
    dev = hip_device
    B, C, H, W, D, M = sl.FULL[0]
    i = inputs(sl.FULL, (170,))
    variant, words = own_plan(sl.FULL, 170, 2)
    expected = launch_into(ops, dev, i, variant, words)
    f1, f2s, Hm, kt = on_device(dev, i, False)
    canary = torch.full((1, 70, H, W), 123.25, device=dev)
    ops.cost_volume_into(f1, f2s, Hm, kt, sl.LO, sl.HI, canary[:, 3:67], variant, work_list=words.to(dev))
    assert bool((canary[:, :3] == 123.25).all()) and bool((canary[:, 67:] == 123.25).all())
    assert torch.equal(canary[:, 3:67], expected)


# ----------------------------------------------------------------------------------------------------------------------
# 6: refusals
# ----------------------------------------------------------------------------------------------------------------------
def test_bad_lists_are_refused_without_a_launch(ops, hip_device):
    """A list on the wrong device, of the wrong dtype or too short: ValueError from ops before anything is launched; the sum-of-absolute-differences
    mode has no tiled kernel, with or without a list: "not supported", the destination untouched."""
    from dvmvs.hip import _capi
    dev = hip_device
    B, C, H, W, D, M = sl.FULL[0]
    i = inputs(sl.FULL, (0,))
    _, words = own_plan(sl.FULL, 0, 2)
    f1, f2s, Hm, kt = on_device(dev, i, False)
    canary = torch.full((B, D, H, W), 7.0, device=dev)
    good = words.to(dev)
    for bad in (words, good.long(), good[:64], good.float()):
        with pytest.raises(ValueError):
            ops.cost_volume_into(f1, f2s, Hm, kt, sl.LO, sl.HI, canary, 2, work_list=bad)
        with pytest.raises(ValueError):
            ops.cost_volume(f1, f2s, Hm, kt, sl.LO, sl.HI, D, True, 2, work_list=bad)
    with pytest.raises(RuntimeError, match="not supported"):
        ops.cost_volume(f1, f2s, Hm, kt, sl.LO, sl.HI, D, False, 2, work_list=good)
    workspace, ws_bytes = ops.sweep_workspace(dev, B, M, H, W, D)
    with torch.cuda.device(dev):
        rc = _capi.lib().dvmvs_cost_volume_planned_fwd(f1.data_ptr(), _capi.pointer_array([t.data_ptr() for t in f2s]), Hm.data_ptr(), kt.data_ptr(),
                                                       canary.data_ptr(), B, M, C, H, W, D, sl.LO, sl.HI, 0, 2, _capi.LAYOUT_NCHW, workspace.data_ptr(), ws_bytes,
                                                       good.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    assert rc != 0 and "not supported" in _capi.lib().dvmvs_error_string(rc).decode()
    torch.cuda.synchronize()
    assert bool((canary == 7.0).all())

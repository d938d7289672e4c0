"""Work lists of the LDS-tiled plane sweep for the tests (tests/test_sweep_work_list_gpu.py, tests/test_sweep_plan.py): the host
planner's list of a keyframe geometry, its items, and a hand-made list in the documented word format
(csrc/sweep_tiled.hip: [0] = number of items, [1] = 0, then per item {tile | batch item << 16, first plane | number of planes << 16}).
Nothing here needs a GPU."""
import numpy as np
import torch

import synthetic as syn

LO, HI = 0.25, 20.0          # depth range of every case
TW, TH, DP = 32, 8, 8        # the tiling of both product configurations (SweepDefault / SweepWide)

# (B, C, H, W, D, M), scale of the full-resolution intrinsics: the shapes of the work-list cases
FULL = ((1, 32, 128, 160, 64, 2), 2.0)
RAGGED = ((1, 32, 61, 83, 37, 2), 320.0 / 83)
TINY = ((1, 5, 33, 47, 10, 2), 320.0 / 47)
ONE_PASS_8 = ((1, 8, 64, 80, 19, 2), 4.0)
ONE_PASS_12 = ((1, 12, 64, 80, 19, 2), 4.0)

# (shape, keyframe index line, forced configuration or 0, the plan cuts (tile, chunk) pairs into plane sub-ranges)
PLAN_CASES = {
    "full-0": (FULL, 0, 0, False), "full-74": (FULL, 74, 0, True), "full-99": (FULL, 99, 0, True), "full-117": (FULL, 117, 0, True),
    "full-141": (FULL, 141, 0, False), "full-170": (FULL, 170, 0, True), "full-202": (FULL, 202, 0, True),
    "full-74-forced2": (FULL, 74, 2, True), "full-170-forced2": (FULL, 170, 2, True), "full-202-forced2": (FULL, 202, 2, True),
    "ragged-170": (RAGGED, 170, 0, True), "ragged-74-forced2": (RAGGED, 74, 2, True),
    "tiny-170-forced2": (TINY, 170, 2, True),
    "one-pass-8": (ONE_PASS_8, 170, 0, True), "one-pass-12": (ONE_PASS_12, 170, 0, True),
}


def poses(lines):
    """(reference poses [B,4,4], [measurement poses [B,4,4]] x M) of keyframe index lines, one batch item per line."""
    index = syn.keyframe_index_lines(2)
    p1 = torch.cat([syn.pose(index[line][0]) for line in lines])
    p2s = [torch.cat([syn.pose(index[line][1][m]) for line in lines]) for m in range(2)]
    return p1, p2s


def intrinsics(lines, k_scale):
    return torch.cat([syn.scaled_K(syn.full_K(), k_scale) for _ in lines])


def matrices(lines, k_scale):
    """Host sweep matrices (Hm [B,M,9], kt [B,M,3]) of keyframe index lines, as tests/test_sweep_plan.py::matrices makes them."""
    from dvmvs import pose_algebra
    p1, p2s = poses(lines)
    return pose_algebra.sweep_matrices_host(p1, p2s, intrinsics(lines, k_scale))


def planned(Hm, kt, H, W, D, forced=0):
    """(variant to launch, int32 host work list) as the frame engine plans them: dvmvs_sweep_plan through ops.sweep_plan_host."""
    from dvmvs.hip import ops
    out = torch.zeros(ops.sweep_work_list_words(Hm.shape[0], H, W, D), dtype=torch.int32)
    variant = ops.sweep_plan_host(Hm, kt, H, W, D, LO, HI, forced, out)
    return variant, out


def parse(words):
    """(n_items, items [n, 2] as int64) of a work list."""
    w = words.cpu().numpy().astype(np.int64) & 0xffffffff
    n = int(w[0])
    return n, w[2:2 + 2 * n].reshape(n, 2)


def tiles_and_chunks(H, W, D):
    return ((W + TW - 1) // TW) * ((H + TH - 1) // TH), (D + DP - 1) // DP


def static_positions(B, H, W, D):
    """Workgroups of a launch without a list = the positions a planned list fills first: (batch, tile, chunk) pairs padded to 8."""
    tiles, chunks = tiles_and_chunks(H, W, D)
    return (B * tiles * chunks + 7) // 8 * 8


def coverage(items, B, H, W, D):
    """How many items hold each (batch, tile, plane)."""
    tiles, _ = tiles_and_chunks(H, W, D)
    cover = np.zeros((B, tiles, D), dtype=np.int64)
    for w0, w1 in items:
        cover[w0 >> 16, w0 & 0xffff, (w1 & 0xffff):(w1 & 0xffff) + (w1 >> 16)] += 1
    return cover


def halved(B, H, W, D):
    """A list nobody planned: every (batch, tile, chunk) with more than 2 planes cut once at lo + (hi - lo + 1) // 2 (the host's own
    rule), the others whole, the items in a fixed shuffled order (an item's position is only its spill slot).  At most 2 x the static
    items, so it fits ops.sweep_work_list_words."""
    from dvmvs.hip import ops
    tiles, chunks = tiles_and_chunks(H, W, D)
    items = []
    for b in range(B):
        for tile in range(tiles):
            for chunk in range(chunks):
                lo, hi = chunk * DP, min(D, chunk * DP + DP)
                cuts = (lo, lo + (hi - lo + 1) // 2, hi) if hi - lo > 2 else (lo, hi)
                for first, last in zip(cuts[:-1], cuts[1:]):
                    items.append((tile | (b << 16), first | ((last - first) << 16)))
    items = np.array(items, dtype=np.int64)[np.random.default_rng(20261019).permutation(len(items))]
    words = np.zeros(ops.sweep_work_list_words(B, H, W, D), dtype=np.int64)
    assert 2 + 2 * len(items) <= len(words)
    words[0] = len(items)
    words[2:2 + 2 * len(items)] = items.reshape(-1)
    return torch.from_numpy(words.astype(np.uint32).view(np.int32).copy())

"""CPU tests of host-side logic of the frame engine that needs no device (dvmvs/frame_host.py, dvmvs/engine.py): the queue that turns a step's input copies into one
launch (CopyQueue), the key of a frame's graph (FrameBody.key), the test for "the announced frame arrived" (DepthEngine._prepared_level), the feature
cache (FeatureCache) and the validation of the fork point.  The copy queue's device entry (dvmvs_copy_batch) is tested on the GPU in
tests/test_sweep_mfma_gpu.py; here the batching op is replaced by a recorder so that the ORDER and GROUPING of the copies can be checked:
copies whose ranges do not touch are grouped, a copy that reads or overwrites a range a queued copy writes (or overwrites one it reads)
goes into a later group, and the result is always what the same copies give when executed one by one in program order."""
import warnings

import pytest
import torch

from dvmvs import engine as engine_module
from dvmvs import frame_host
from dvmvs.engine import CopyQueue, DepthEngine, FeatureCache, FrameBody


class _Recorder:
    """Stands in for dvmvs.hip.ops: everything dense is 'batchable', a batch is executed pair by pair and its size recorded."""

    def __init__(self):
        self.batches = []

    def batchable(self, dst, src):
        return dst.shape == src.shape and dst.is_contiguous() and src.is_contiguous() and dst.numel() % 4 == 0

    def copy_batch(self, pairs):
        self.batches.append(len(pairs))
        spans = [((d.data_ptr(), d.data_ptr() + 4 * d.numel()), (s.data_ptr(), s.data_ptr() + 4 * s.numel())) for d, s in pairs]
        for i, (di, si) in enumerate(spans):      # the entry's contract: no write range touches another pair's write or read range
            for j, (dj, sj) in enumerate(spans):
                if i != j:
                    assert not (di[0] < dj[1] and dj[0] < di[1]) and not (di[0] < sj[1] and sj[0] < di[1]), "dependent copies in one launch"
        snapshot = [(d, s.clone()) for d, s in pairs]      # (a launch reads every source before any of its writes is visible to the others)
        for d, s in snapshot:
            d.copy_(s)


def _open_queue(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(frame_host, "_ops", rec)
    queue = CopyQueue()
    queue.open()
    return queue, rec


def test_independent_copies_become_one_launch(monkeypatch):
    queue, rec = _open_queue(monkeypatch)
    pool = torch.zeros(6, 64)
    srcs = [torch.full((64,), float(i + 1)) for i in range(4)]
    for i in range(4):
        queue.add(pool[i], srcs[i])
    assert rec.batches == []                                  # nothing issued before the flush
    queue.flush()
    assert rec.batches == [4] and queue.pending == []
    for i in range(4):
        assert torch.equal(pool[i], srcs[i])
    queue.add(pool[4], srcs[0])                             # a single queued copy is a plain copy_
    queue.flush()
    assert rec.batches == [4] and torch.equal(pool[4], srcs[0])


def test_dependent_copies_are_split_in_program_order(monkeypatch):
    """slot <- features; buffer <- slot (read after write), slot <- other (write after read / write after write): the later copy starts a new
    group, and the outcome equals sequential execution."""
    queue, rec = _open_queue(monkeypatch)
    g = torch.Generator().manual_seed(0)
    mem = torch.zeros(8, 32)
    a, b = torch.randn(32, generator=g), torch.randn(32, generator=g)
    program = [(mem[0], a), (mem[1], mem[0]), (mem[0], b), (mem[2], mem[1]), (mem[3], a), (mem[0], mem[3])]
    expect = torch.zeros(8, 32)
    for (d, s_) in program:
        exp_d = expect[(d.data_ptr() - mem.data_ptr()) // (32 * 4)]
        exp_s = s_ if s_.data_ptr() < mem.data_ptr() or s_.data_ptr() >= mem.data_ptr() + mem.numel() * 4 else expect[(s_.data_ptr() - mem.data_ptr()) // (32 * 4)]
        exp_d.copy_(exp_s.clone())
    for d, s_ in program:
        queue.add(d, s_)
    queue.flush()
    assert torch.equal(mem, expect)
    assert rec.batches == [3]      # (m0 <- b, m2 <- m1, m3 <- a) went out together; the dependent ones one by one -- the recorder checks every launch


def test_outside_a_step_and_for_odd_tensors_the_copy_is_immediate(monkeypatch):
    queue, rec = _open_queue(monkeypatch)
    dst, src = torch.zeros(2, 6), torch.ones(2, 6)
    queue.close()                                               # not inside step(): executed at once
    queue.add(dst, src)
    assert torch.equal(dst, src) and rec.batches == []
    queue.open()
    queued_dst, queued_src = torch.zeros(8), torch.arange(8.0)
    queue.add(queued_dst, queued_src)
    odd_dst, odd_src = torch.zeros(3), torch.ones(3)          # not a multiple of 4 elements: flushes the queue, then copies directly
    queue.add(odd_dst, odd_src)
    assert torch.equal(queued_dst, queued_src) and torch.equal(odd_dst, odd_src) and queue.pending == []
    for i in range(9):                                        # the entry takes eight copies: the ninth starts a new launch
        queue.add(torch.zeros(4), torch.ones(4))
    assert rec.batches == [8] and len(queue.pending) == 1


# ---- FrameBody.key -----------------------------------------------------------------------------------------------------------
def test_frame_body_key_masks_only_the_stages_that_do_not_run():
    body = FrameBody(n_meas=2, has_previous=True, sweep_variant=6, parity=1, have=1, give=2, n_meas_next=2, next_variant=3)
    assert tuple(body) == (2, True, 6, 1, 1, 2, 2, 3) and body[4] == body.have and body[5] == body.give      # (a plain tuple to its readers)
    assert body.key() == body and isinstance(body.key(), FrameBody)      # have < 2 and give == 2: every stage runs
    assert body._replace(have=0).key() == body._replace(have=0)
    # the frame's own sweep + encoder ran a frame ahead: its measurement count and sweep configuration do not tell graphs apart
    done = body._replace(have=2)
    assert done.key() == done._replace(n_meas=1).key() == done._replace(sweep_variant=2).key() == done._replace(n_meas=0, sweep_variant=0)
    assert body.key() != body._replace(n_meas=1).key() and body.key() != body._replace(sweep_variant=2).key()      # (they do while it runs)
    # the next frame's sweep does not run: its measurement count and configuration are masked
    for give in (0, 1):
        short = body._replace(give=give)
        assert short.key() == short._replace(n_meas_next=1).key() == short._replace(next_variant=5).key() == short._replace(n_meas_next=0, next_variant=0)
    assert body.key() != body._replace(n_meas_next=1).key() and body.key() != body._replace(next_variant=5).key()
    # every other field tells graphs apart, whatever runs
    for base in (body, done, body._replace(give=1), done._replace(give=0)):
        others = [base._replace(has_previous=not base.has_previous), base._replace(parity=1 - base.parity),
                  base._replace(have=(base.have + 1) % 3), base._replace(give=(base.give + 1) % 3)]
        assert all(other.key() != base.key() for other in others)
    assert len({body.key(): 0, tuple(body): 1}) == 1      # (hashes and compares as the tuple it is: what the graph dict is read by)


# ---- the announced frame ------------------------------------------------------------------------------------------------------
def _announced(image, level=1):
    """A bare engine to which frame 7 was announced as ``image`` for buffer set 1, prepared to ``level``."""
    eng = DepthEngine.__new__(DepthEngine)
    eng.direct, eng.lookahead_rejected = True, 0
    eng._prefetched = dict(frame_id=7, parity=1, level=level, sweep_variant=6, image=image, image_version=image._version)
    pose, meas, K = torch.eye(4).reshape(1, 4, 4), [torch.eye(4).reshape(1, 4, 4) * 2.0, torch.eye(4).reshape(1, 4, 4) * 3.0], torch.eye(3).reshape(1, 3, 3)
    if level == 2:
        eng._prefetched.update(pose=pose.clone(), measurement_ids=[5, 6], full_K=K.clone(), measurement_poses=[m.clone() for m in meas])
    level_of = lambda img, frame_id=7, parity=1, ids=(5, 6), p=pose, m=meas, k=K: eng._prepared_level(frame_id, parity, img, p, list(ids), m, k)
    return eng, level_of, (pose, meas, K)


def test_only_the_very_tensor_that_was_announced_is_accepted():
    image = torch.arange(2.0 * 3 * 4 * 6).reshape(2, 3, 4, 6)
    eng, level_of, _ = _announced(image)
    with warnings.catch_warnings():
        warnings.simplefilter("error")      # (none of these warns)
        assert level_of(image) == 1
        assert level_of(image, frame_id=8) == 0 and level_of(image, frame_id=None) == 0 and level_of(image, parity=0) == 0
        assert eng.lookahead_rejected == 0      # (another frame, another buffer set: nothing that was announced went missing)
    strided = image.transpose(2, 3).transpose(2, 3)[:, :, ::2]      # same storage and address, other strides
    assert strided.data_ptr() == image.data_ptr() and strided.stride() != image.stride()
    with pytest.warns(RuntimeWarning) as caught:
        assert level_of(image.clone()) == 0 and eng.lookahead_rejected == 1
        assert level_of(strided) == 0 and eng.lookahead_rejected == 2
    assert len(caught) == 1      # two rejections, one warning
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert level_of(image) == 1      # (a rejection forgets nothing)
        image.add_(1.0)                  # modified in place since it was announced: a version bump
        assert level_of(image) == 0 and eng.lookahead_rejected == 3
    assert DepthEngine._is_announced_tensor(dict(image=image, image_version=image._version), image)
    assert not DepthEngine._is_announced_tensor(dict(image=image, image_version=image._version), image.clone())


def test_the_second_level_needs_the_announced_ids_poses_and_intrinsics():
    image = torch.zeros(1, 3, 4, 6)
    eng, level_of, (pose, meas, K) = _announced(image, level=2)
    assert level_of(image) == 2
    assert level_of(image, ids=(5, 4)) == 1
    assert level_of(image, p=pose + 1e-3) == 1
    assert level_of(image, m=[meas[0], meas[1] + 1e-3]) == 1 and level_of(image, m=meas[:1], ids=(5,)) == 1
    assert level_of(image, k=K * 1.5) == 1
    assert level_of(image) == 2 and eng.lookahead_rejected == 0
    assert _announced(image, level=1)[1](image) == 1      # (what was prepared to level 1 stays level 1)


# ---- the feature cache --------------------------------------------------------------------------------------------------------
def _cache(monkeypatch, channels_last_entries=False):
    queue, rec = _open_queue(monkeypatch)
    return FeatureCache(3, torch.device("cpu"), channels_last_entries), queue


def test_feature_cache_evicts_the_least_recently_used_entry_and_reuses_its_slot(monkeypatch):
    cache, queue = _cache(monkeypatch)
    maps = {i: torch.full((1, 4, 6, 5), float(i)) for i in range(1, 6)}
    for i in (1, 2, 3):
        cache.remember(i, maps[i], queue.add)
    assert tuple(cache.pool.shape) == (4, 1, 4, 6, 5) and sorted(cache.free + list(cache.slot.values())) == [0, 1, 2, 3] and len(cache.free) == 1
    first = cache.slot[1]
    cache.remember(4, maps[4], queue.add)                    # the fourth: frame 1, the least recently used, leaves
    assert 1 not in cache and all(i in cache for i in (2, 3, 4)) and 1 not in cache.slot
    assert cache.slot[4] == first and cache.free == [3]     # its slot went back to the free list, from where the newcomer took it
    assert cache.lookup(2) is cache[2]                       # a lookup refreshes: now 3 is the least recently used
    cache.remember(5, maps[5], queue.add)
    assert 3 not in cache and all(i in cache for i in (2, 4, 5))
    where = cache[4].data_ptr()
    cache.remember(4, maps[1], queue.add)                    # an id that is cached keeps its slot (and becomes the most recent)
    assert cache[4].data_ptr() == where and list(cache.entries) == [2, 5, 4] and sorted(cache.free + list(cache.slot.values())) == [0, 1, 2, 3]
    queue.flush()
    assert torch.equal(cache[2], maps[2]) and torch.equal(cache[5], maps[5]) and torch.equal(cache[4], maps[1])
    cache.remember(2, cache[2], queue.add)                   # the entry's own buffer: nothing to copy
    assert queue.pending == [] and torch.equal(cache[2], maps[2])


def test_feature_cache_rebuilds_its_pool_for_another_shape_and_clear_frees_every_slot(monkeypatch):
    cache, queue = _cache(monkeypatch)
    for i in (1, 2, 3):
        cache.remember(i, torch.full((1, 4, 6, 5), float(i)), queue.add)
    queue.flush()
    cache.clear()
    assert 1 not in cache and len(cache.entries) == 0 and cache.free == [3, 2, 1, 0] and cache.slot == {}
    cache.remember(1, torch.ones(1, 4, 6, 5), queue.add)
    cache.remember(9, torch.ones(1, 4, 3, 5), queue.add)      # another shape: a new pool, and nothing of the old one is kept
    queue.flush()
    assert tuple(cache.pool.shape) == (4, 1, 4, 3, 5) and list(cache.entries) == [9] and cache.free == [3, 2, 1] and cache.slot == {9: 0}
    assert torch.equal(cache[9], torch.ones(1, 4, 3, 5))
    kept = torch.ones(1, 4, 6, 5).permute(0, 1, 3, 2)         # not contiguous, no channels-last pool: kept as it is
    cache.remember(10, kept, queue.add)
    assert cache[10] is kept and 10 not in cache.slot


def test_feature_cache_hands_out_channels_last_slots(monkeypatch):
    cache, queue = _cache(monkeypatch, channels_last_entries=True)
    maps = [torch.randn(1, 4, 6, 5, generator=torch.Generator().manual_seed(i)).contiguous(memory_format=torch.channels_last) for i in range(4)]
    for i, m in enumerate(maps):
        cache.remember(i, m, queue.add)
        assert cache[i].is_contiguous(memory_format=torch.channels_last) and tuple(cache[i].shape) == (1, 4, 6, 5)
    queue.flush()
    assert 0 not in cache and all(torch.equal(cache[i], maps[i]) for i in (1, 2, 3))


# ---- the fork point ------------------------------------------------------------------------------------------------------------
def test_fork_point_is_validated():
    assert [engine_module._fork_point(v) for v in ("-1", "0", "4", 1)] == [-1, 0, 4, 1]
    for bad in ("-2", "5", "behind the sweep", "1.5", None):
        with pytest.raises(ValueError):
            engine_module._fork_point(bad)

"""The frame engine's host-side parts that need no device (tests/test_engine_host_logic.py): the description of a frame body and the key of its
graph (``FrameBody``), the queue that turns a step's input copies into one launch (``CopyQueue``) and the keyframe feature cache
(``FeatureCache``)."""
from collections import OrderedDict
from typing import NamedTuple

import torch

from dvmvs.hip import ops as _ops


class FrameBody(NamedTuple):
    """What one call of the frame body computes (DepthEngine._frame_body's arguments): ``have`` = how much of the frame the previous step
    prepared, ``give`` = how much of the next frame this one computes (0 nothing, 1 reference features, 2 also sweep + encoder)."""
    n_meas: int
    has_previous: bool
    sweep_variant: int
    parity: int
    have: int
    give: int
    n_meas_next: int
    next_variant: int

    def key(self):
        """The body as the key of its captured graph: stages that do not run in this graph do not tell graphs apart."""
        own, ahead = self.have < 2, self.give == 2
        return self._replace(n_meas=self.n_meas if own else 0, sweep_variant=self.sweep_variant if own else 0,
                             n_meas_next=self.n_meas_next if ahead else 0, next_variant=self.next_variant if ahead else 0)


def _store_measurement_map(dst, src):
    """``dst`` = ``src``; an NCHW map into a channels-last buffer through the transposing kernel (torch's strided copy writes 4 bytes per
    128-byte line)."""
    if src.stride() == dst.stride() or not (src.is_contiguous() and dst.is_contiguous(memory_format=torch.channels_last) and src.shape[1] % 4 == 0 and src.shape[1] <= 64):
        dst.copy_(src)      # (the frame path: channels-last into channels-last)
    else:
        _ops.nchw_to_nhwc_into(src, dst)


class CopyQueue:
    """A step's flat input copies -- this keyframe's features into the feature cache, the measurement maps into the sweep's buffers, the images
    into their homes: four runtime copies of 0.6 - 1 MB in front of every frame graph, 5 us each on the device and as much again on the host --
    collected while the queue is open and issued as ONE launch (dvmvs_copy_batch) before the frame's parameters go up.  Closed (outside
    ``step``), or for a copy the batch entry does not take, ``add`` copies at once."""

    def __init__(self):
        self.pending = None      # None: closed; a list of (dst, src) while open

    def open(self):
        self.pending = []

    def close(self):
        """Closes the queue and hands over what is still queued (``issue`` it, alone or with the parameter block)."""
        pending, self.pending = self.pending, None
        return pending

    def add(self, dst, src):
        """``dst`` = ``src`` (see _store_measurement_map).  A copy that touches a range a queued copy writes (or writes one a queued copy
        reads) flushes the queue first; so does the eighth copy (what one launch takes)."""
        queue = self.pending
        if queue is None or not _ops.batchable(dst, src):
            self.flush()
            _store_measurement_map(dst, src)
            return
        nbytes = 4 * dst.numel()
        d0, s0 = dst.data_ptr(), src.data_ptr()
        for qd, qs in queue:
            q0, r0, qn = qd.data_ptr(), qs.data_ptr(), 4 * qd.numel()
            if (d0 < q0 + qn and q0 < d0 + nbytes) or (s0 < q0 + qn and q0 < s0 + nbytes) or (d0 < r0 + qn and r0 < d0 + nbytes):
                self.flush()
                break
        queue.append((dst, src))
        if len(queue) == 8:
            self.flush()

    def flush(self):
        self.issue(self.pending)

    @staticmethod
    def issue(pairs):
        """Executes and forgets the copies of ``pairs`` (a list, or None): one plain copy, or one batched launch."""
        if pairs:
            if len(pairs) == 1:
                pairs[0][0].copy_(pairs[0][1])
            else:
                _ops.copy_batch(pairs)
            pairs.clear()


class FeatureCache:
    """frame id -> a keyframe's half-resolution features, least recently used first.  The entries live in a pool of ``cache_size + 1`` buffers
    allocated once per entry shape: a ``clone()`` per keyframe made the first ``cache_size`` frames of every run pay a device allocation each
    (hipMalloc synchronises: a 20-step run measured 1.7 ms per frame where 100 steps measured 1.39).  ``channels_last_entries``: the pool's
    buffers are channels-last (what the MFMA sweep reads); without it a non-contiguous entry is kept as it is, outside the pool."""

    def __init__(self, cache_size, device, channels_last_entries):
        self.cache_size, self.device, self.channels_last_entries = cache_size, device, channels_last_entries
        self.entries = OrderedDict()      # frame id -> features (a buffer of the pool)
        self.pool, self.free, self.slot = None, [], {}      # [cache_size + 1, *entry shape]; free pool indices; frame id -> pool index

    def __contains__(self, frame_id):
        return frame_id in self.entries

    def __getitem__(self, frame_id):
        return self.entries[frame_id]

    def lookup(self, frame_id):
        """The entry, now the most recently used one."""
        self.entries.move_to_end(frame_id)
        return self.entries[frame_id]

    def clear(self):
        self.entries.clear()
        if self.pool is not None:
            self.free = list(range(self.pool.shape[0] - 1, -1, -1))
        self.slot = {}

    def remember(self, frame_id, half, copy):
        """Caches ``half`` under ``frame_id``: into the id's own slot if it has one, else into a free one (the least recently used entry gives
        its slot back first); the values go there through ``copy(dst, src)``.  An entry of another shape rebuilds the pool and empties the cache."""
        if not half.is_contiguous() and not self.channels_last_entries:      # (channels-last engines keep their maps as they are: the sweep reads them as NHWC)
            self.entries[frame_id] = half
            while len(self.entries) > self.cache_size:
                self.slot.pop(self.entries.popitem(last=False)[0], None)
            return
        if self.pool is None or tuple(self.pool.shape[1:]) != tuple(half.shape):
            if self.channels_last_entries and half.dim() == 4:      # channels-last entries (what the sweep reads): [n, S, H, W, C] storage, [n, S, C, H, W] view
                S_, C_, H_, W_ = half.shape
                self.pool = torch.empty((self.cache_size + 1, S_, H_, W_, C_), device=self.device, dtype=torch.float32).permute(0, 1, 4, 2, 3)
            else:
                self.pool = torch.empty((self.cache_size + 1,) + tuple(half.shape), device=self.device, dtype=torch.float32)
            self.clear()
        if frame_id in self.entries:
            buffer = self.entries.pop(frame_id)
        else:
            while len(self.entries) >= self.cache_size:      # least recently used entry out, its buffer back to the pool
                self.free.append(self.slot.pop(self.entries.popitem(last=False)[0]))
            buffer = self.pool[self.free[-1]]
            self.slot[frame_id] = self.free.pop()
        if buffer.data_ptr() != half.data_ptr():
            copy(buffer, half)
        self.entries[frame_id] = buffer

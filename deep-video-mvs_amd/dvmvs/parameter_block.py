"""The frame's parameter block: the small matrices of one frame -- sweep matrices, the two relative poses, intrinsics, poses -- and the sweep's
work list in ONE device buffer with fixed offsets (captured graphs keep pointing at the right place), evaluated on the host with the reference's
own fp32 expressions (``dvmvs.pose_algebra``) and sent up with one copy per frame out of a pinned staging slot.  The host half -- layout, mirror,
evaluation -- needs no device (tests/test_host_scaling.py); ``allocate`` adds the device buffer, its named views and the staging slot."""
import os
import time

import torch

from dvmvs import pose_algebra as _pose_algebra
from dvmvs import utils as _utils
from dvmvs.frame_host import CopyQueue
from dvmvs.hip import ops as _ops

_MAX_MEAS = 8            # DVMVS_MAX_MEASUREMENTS of the C ABI


class ParameterBlock:
    """Layout, host mirror, device buffer and upload of a frame's parameters, and the thread that plans the next frame's block ahead."""

    def __init__(self, sequences, height, width, n_depth_levels, min_depth, max_depth, pose_algebra, sweep_work_list, sweep_mfma, is_fusionnet):
        self.sequences, self.height, self.width, self.n_depth_levels = sequences, height, width, n_depth_levels
        self.min_depth, self.max_depth, self.pose_algebra = min_depth, max_depth, pose_algebra
        self.sweep_work_list, self.sweep_mfma, self.is_fusionnet = sweep_work_list, sweep_mfma, is_fusionnet
        self.offsets, self.total = self._parameter_layout(sequences, height, width, n_depth_levels)
        self.mirror = torch.zeros(self.total, dtype=torch.float32)      # host mirror of the block: a step rewrites only its own regions
        self.device, self.params, self.views = None, None, {}      # see allocate
        self._staging, self._staging_event, self._staging_is_visible = None, None, None
        self._planner, self._planned, self._mirror_ahead = None, None, None      # see plan_ahead
        self._switch_interval_before = None
        self.planned_frames_used = 0
        self.ring_wait_seconds = 0.0     # time upload() spent waiting for the device at the staging slot (NOT host work: bench.py subtracts it)

    @staticmethod
    def _parameter_layout(S, H, W, n_depth_levels):
        """({name: (offset, floats)}, total floats) of the frame's parameter block: one device buffer, one upload per frame, fixed offsets so that
        captured graphs keep pointing at the right place; Hm / kt are sized for the ABI's maximum number of measurement frames."""
        items = _ops.sweep_work_list_words(S, H // 2, W // 2, n_depth_levels)
        sizes = [("Hm", S * _MAX_MEAS * 9), ("kt", S * _MAX_MEAS * 3), ("reproject_T", S * 16), ("lstm_T", S * 16),
                 ("full_K", S * 9), ("half_K", S * 9), ("lstm_K", S * 9), ("pose", S * 16), ("prev_pose", S * 16),
                 ("meas_pose", _MAX_MEAS * S * 16),
                 # the sweep's work list (32-bit words, planned on the host per frame: dvmvs_sweep_work_list) rides in the same upload
                 ("sweep_items", items),
                 # the sweep parameters of the OTHER buffer set (look-ahead: the next frame's sweep runs during this frame)
                 ("Hm1", S * _MAX_MEAS * 9), ("kt1", S * _MAX_MEAS * 3), ("sweep_items1", items)]
        offsets, total = {}, 0
        for name, n in sizes:
            offsets[name] = (total, n)
            total += n
        return offsets, (total + 3) // 4 * 4      # (whole float4: the upload can ride in the frame's copy batch)

    # ---- device half --------------------------------------------------------------------------------------------------------
    def allocate(self, device):
        """The device buffer, its named views (``views``: what the frame body's kernels read) and the pinned staging slot with its event."""
        S, self.device = self.sequences, device
        self.params = torch.zeros(self.total, device=device, dtype=torch.float32)
        view = lambda name, *shape: self.params[self.offsets[name][0]:self.offsets[name][0] + self.offsets[name][1]].view(*shape)
        self.views = dict(reproject_T=view("reproject_T", S, 4, 4), lstm_T=view("lstm_T", S, 4, 4),
                          full_K=view("full_K", S, 3, 3), half_K=view("half_K", S, 3, 3), lstm_K=view("lstm_K", S, 3, 3),
                          pose=view("pose", S, 4, 4), prev_pose=view("prev_pose", S, 4, 4),
                          meas_pose=[view("meas_pose", _MAX_MEAS, S, 4, 4)[i] for i in range(_MAX_MEAS)])
        # The pinned staging slot: the host waits for the slot's previous upload to have executed before it overwrites it, so the number of slots is
        # how many frames the host may run ahead of the device.
        # Round 3: with 8 the host (0.7 ms per step) raced up to 8 graph launches ahead of the device (1.3 ms per frame) and every 10-20 frames one
        # frame took 2.5-5 ms instead of 1.3 on the device -- the deeper the queue of launched graphs, the more such stalls (2 / 3 / 8 / 64 slots:
        # 1 / 2 / 4 / 6 of them in 70 frames, tools/step_times_probe.py) -- hence TWO.  Round 5: the one stall that was left (a 5.6-7.4 ms device
        # gap four steps after every full device synchronisation, i.e. inside the timed steps of a short benchmark run: 830-910 instead of
        # 1 160-1 180 frames/s on the driver's command) is the same effect -- a frame's graph launched again while its previous launch (two frames
        # back: frames alternate between two graphs) is still queued or running.  With ONE slot the host is at most one frame ahead, a graph is
        # never in flight twice, and the stall is gone at the same steady-state rate (3 / 2 / 1 slots: 2 / 1 / 0 stalls in 20 steps; 100 steps:
        # 1 239 frames/s): the host's 0.75 ms per step still overlap the device's 0.8 ms frame completely.
        self._staging, self._staging_event = torch.zeros(self.total, dtype=torch.float32).pin_memory(), torch.cuda.Event()

    def sweep_views(self, n_meas, index=0):
        """Hm [S,n_meas,9] and kt [S,n_meas,3] views of the parameter buffer (contiguous prefixes of their regions) of buffer set ``index``."""
        S, p = self.sequences, self.params
        suffix = "1" if index else ""
        o_h, o_k = self.offsets["Hm" + suffix][0], self.offsets["kt" + suffix][0]
        return p[o_h:o_h + S * n_meas * 9].view(S, n_meas, 9), p[o_k:o_k + S * n_meas * 3].view(S, n_meas, 3)

    def sweep_items(self, index=0):
        """The device copy of a frame's work list (a fixed region of the parameter buffer per buffer set: captured graphs keep pointing at it)."""
        if not self.sweep_work_list:
            return None
        o, n = self.offsets["sweep_items1" if index else "sweep_items"]
        return self.params.view(torch.int32)[o:o + n]

    def upload(self, n_meas, pose, measurement_poses, full_K, previous_pose, no_previous, index=0, own_sweep=True, next_frame=None, pending_copies=None):
        """Evaluates the frame's small matrices on the host (reference mode) and sends them, the intrinsics and the poses to
        the device with ONE asynchronous copy out of the pinned staging slot.  The slot's previous copy (issued one frame ago)
        must have executed before it is overwritten: its event is waited for.

        ``previous_pose`` / ``no_previous``: the engine's host copy of the previous frame's pose and which sequences have none;
        ``index``: the buffer set of this frame (its sweep parameters live in that set's region); ``own_sweep`` False: this frame's
        sweep already ran (look-ahead), its region is left as it is; ``next_frame`` = (pose, measurement poses) of the NEXT frame whose
        sweep runs during this one: its matrices / work list go into the other set's region.  Regions a step does not rewrite keep
        their contents through the host mirror of the block.
        Returns (the host pose that becomes "the previous pose" -- committed by step() only after the frame was launched, so that a
        frame that raises leaves (h, c, previous depth, previous pose) those of one frame --, this frame's sweep configuration or
        None, the next frame's or None)."""
        try:
            planned = self._take_planned(n_meas, pose, measurement_poses, full_K, previous_pose, no_previous, index, own_sweep, next_frame)
            if planned is not None:
                result = planned
            else:
                result = self.evaluate(self.mirror, n_meas, pose, measurement_poses, full_K, previous_pose, no_previous, index, own_sweep, next_frame)
        except BaseException:
            CopyQueue.issue(pending_copies)      # (they belong to cache entries that are already registered: written before the error leaves)
            raise
        staging, event = self._staging, self._staging_event
        t_wait = time.perf_counter()
        event.synchronize()      # (one staging slot: the host runs at most one frame ahead of the device, so in steady state this is where a step waits for it)
        self.ring_wait_seconds += time.perf_counter() - t_wait
        staging.copy_(self.mirror)
        with torch.cuda.device(self.device):     # the slot's guard must be recorded on the engine's device, whichever is current
            params = self.params
            if pending_copies and len(pending_copies) < 8 and self._staging_visible():
                # the block goes up in the SAME launch as the frame's input copies (round 6): the copy kernel reads the pinned staging slot through
                # its device-visible address -- the runtime's own copy of a pinned buffer is a blit kernel too (__amd_rocclr_copyBuffer), one
                # launch more per frame
                _ops.copy_batch(pending_copies + [(params, staging)])
            else:
                CopyQueue.issue(pending_copies)
                params.copy_(staging, non_blocking=True)
            event.record(torch.cuda.current_stream(self.device))
        return result

    def _staging_visible(self):
        """Whether kernels on the engine's device may read the pinned staging slot directly (asked once: dvmvs_host_pointer_device_visible)."""
        if self._staging_is_visible is None:
            from dvmvs.hip import _capi
            key = self._staging.data_ptr()
            self._staging_is_visible = bool(self._staging.is_pinned() and key % 16 == 0 and _capi.lib().dvmvs_host_pointer_device_visible(key))
        return self._staging_is_visible

    # ---- host half ----------------------------------------------------------------------------------------------------------
    def evaluate(self, mirror, n_meas, pose, measurement_poses, full_K, previous_pose, no_previous, index, own_sweep, next_frame):
        """The host half of ``upload``: evaluates the matrices, the sweep configuration and the work list and writes
        them into ``mirror`` (a host copy of the parameter block).  Touches no state of the block -- it also runs on the planning thread, a
        frame ahead, into a second mirror (``plan_ahead``)."""
        S = self.sequences
        host = _pose_algebra.to_host
        pose, full_K = host(pose).reshape(S, 4, 4), host(full_K).reshape(S, 3, 3)
        measurement_poses = [host(p).reshape(S, 4, 4) for p in measurement_poses]
        half_K, lstm_K = full_K.clone(), full_K.clone()
        half_K[:, 0:2, :] = half_K[:, 0:2, :] / 2.0       # run-testing.py:139-140
        lstm_K[:, 0:2, :] = lstm_K[:, 0:2, :] / 32.0      # run-testing.py:142-143
        # A sequence without a previous frame (S > 1 runs every sequence through the previous-frame path) gets the identity as
        # relative pose: its previous depth is all zero, and under the identity every zero-depth point stays at z = 0, which the
        # splat never writes -- an exactly empty depth estimate, as on the reference's first-frame path.
        previous = torch.where(no_previous.view(S, 1, 1), pose, previous_pose)

        def put(name, tensor):
            o, n = self.offsets[name]
            flat = tensor.reshape(-1)
            mirror[o:o + flat.numel()].copy_(flat)

        def put_sweep(region, ref_pose, meas_poses):
            """Sweep matrices, configuration and work list of one frame into buffer set ``region``'s part of the block."""
            suffix = "1" if region else ""
            Hm, kt = _pose_algebra.sweep_matrices_host(ref_pose, meas_poses, half_K)
            put("Hm" + suffix, Hm)
            put("kt" + suffix, kt)
            # which sweep configuration suits this keyframe geometry and its work list: decided here, on the host copies, in one walk
            # over the (tile, chunk) pairs (one graph per configuration)
            variant = _utils.COST_VOLUME_VARIANT
            if self.sweep_work_list:
                o, n = self.offsets["sweep_items" + suffix]
                variant = _ops.sweep_plan_host(Hm, kt, self.height // 2, self.width // 2, self.n_depth_levels, self.min_depth, self.max_depth,
                                               variant if variant in (2, 3, 4, 5) else 0, mirror.view(torch.int32)[o:o + n], allow_mfma=self.sweep_mfma)
            elif variant == 0:
                variant = _utils.sweep_variant((Hm, kt), self.height // 2, self.width // 2, self.n_depth_levels, self.min_depth, self.max_depth)
            return variant

        sweep_variant = _utils.COST_VOLUME_VARIANT if own_sweep else None
        next_variant = None
        if self.pose_algebra == "reference":
            if own_sweep:
                sweep_variant = put_sweep(index, pose, measurement_poses)
            if next_frame is not None:
                next_variant = put_sweep(1 - index, host(next_frame[0]).reshape(S, 4, 4), [host(p).reshape(S, 4, 4) for p in next_frame[1]])
            if self.is_fusionnet:
                eye = torch.eye(4).expand(S, 4, 4)
                if bool(no_previous.all()):      # nothing to relate to: the identity, exactly (see above)
                    reproject_T = lstm_T = eye
                else:
                    fresh = no_previous.view(S, 1, 1)
                    reproject_T = torch.where(fresh, eye, _pose_algebra.relative_pose_host(pose, previous))   # utils.py:121
                    lstm_T = torch.where(fresh, eye, _pose_algebra.relative_pose_host(previous, pose))        # convlstm.py:30
                put("reproject_T", reproject_T)
                put("lstm_T", lstm_T)
        put("full_K", full_K)
        put("half_K", half_K)
        put("lstm_K", lstm_K)
        put("pose", pose)
        put("prev_pose", previous)
        put("meas_pose", torch.stack(measurement_poses))
        return pose.clone(), sweep_variant, next_variant

    # ---- planning a frame ahead on a second host thread -----------------------------------------------------------------
    def plan_ahead(self, n_meas, pose, measurement_poses, full_K, previous_pose, index):
        """Starts evaluating the NEXT frame's parameter block (pose algebra, sweep configuration, work list: ~0.3 ms of small host
        operations) on the planning thread, while this thread is inside hipGraphLaunch (0.4 ms, GIL released).  With the direct
        convolutions a frame takes the device 0.8 ms and took the host 0.9: the host had become the bound.  The next ``upload`` takes the
        result if it is called with these very poses (else it evaluates its own, as before): same functions on the same inputs."""
        if self._planner is None:
            from concurrent.futures import ThreadPoolExecutor
            self._planner = ThreadPoolExecutor(max_workers=1, thread_name_prefix="dvmvs-plan")
            # Two Python threads share the interpreter lock: a thread that wants it asks the holder to drop it only after the switch
            # interval -- 5 ms by default, six frames of device time.  A few steps into every run this thread came back from a graph launch
            # while the planning thread was mid-block and sat out the full interval (one 5.6-6.5 ms device gap in the first ten steps of every
            # short run; none with DVMVS_PLAN_AHEAD=0).  0.1 ms bounds the hand-over; DVMVS_SWITCH_INTERVAL overrides (seconds, 0 = leave it).
            # OPT-IN since round 6 (a library must not change the embedding program's interpreter behaviour): bench.py sets
            # DVMVS_SWITCH_INTERVAL=1e-4; unset = the interpreter's interval stays as it is.  close() restores it.
            import sys
            wanted = float(os.environ.get("DVMVS_SWITCH_INTERVAL", "0"))
            if wanted > 0.0 and sys.getswitchinterval() > wanted:
                self._switch_interval_before = sys.getswitchinterval()
                sys.setswitchinterval(wanted)
            self._mirror_ahead = torch.zeros_like(self.mirror)
        no_previous = torch.zeros(self.sequences, dtype=torch.bool)
        inputs = (pose, list(measurement_poses), full_K)
        future = self._planner.submit(self.evaluate, self._mirror_ahead, n_meas, pose, measurement_poses, full_K,
                                      previous_pose, no_previous, index, True, None)
        self._planned = (inputs, previous_pose, index, future)

    def close(self):
        """Stops the planning thread and puts the interpreter's switch interval back (if DVMVS_SWITCH_INTERVAL made this block change it)."""
        if self._planner is not None:
            self._planner.shutdown(wait=True)
            self._planner, self._planned = None, None
        if self._switch_interval_before is not None:
            import sys
            sys.setswitchinterval(self._switch_interval_before)
            self._switch_interval_before = None

    def _take_planned(self, n_meas, pose, measurement_poses, full_K, previous_pose, no_previous, index, own_sweep, next_frame):
        """The block planned a frame ahead, copied into the mirror, if it was planned for exactly this call; else None."""
        planned, self._planned = self._planned, None
        if planned is None:
            return None
        (p_pose, p_meas, p_K), p_previous, p_index, future = planned
        try:
            result = future.result()          # (also when it is not used: the second mirror must be idle before the next plan)
        except Exception:
            return None                       # evaluated again by the caller, which raises in the caller's thread
        same = lambda a, b: a is b or (tuple(a.shape) == tuple(b.shape) and a.device == b.device and torch.equal(a, b))
        if not (own_sweep and next_frame is None and p_index == index and len(p_meas) == n_meas == len(measurement_poses)
                and not bool(no_previous.any()) and same(p_pose, pose) and same(p_K, full_K)
                and all(same(a, b) for a, b in zip(p_meas, measurement_poses)) and torch.equal(p_previous, previous_pose)):
            return None
        self.mirror.copy_(self._mirror_ahead)
        self.planned_frames_used += 1
        return result

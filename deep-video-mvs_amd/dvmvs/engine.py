"""Per-keyframe forward orchestration for pairnet / fusionnet on one MI355X.

The reference keeps this logic inside its scripts (/root/reference/dvmvs/fusionnet/run-testing.py:151-204,
pairnet/run-testing.py:136-166); here it is a small class so that the same frame contract can be driven by the
test runner, the benchmark and the sequence-sharded multi-GPU runner:

    features(measurement frames) , features(reference) -> fused plane-sweep cost volume (HIP) -> encoder
      -> [fusionnet] previous depth splatted into the current view (HIP) -> ConvLSTM (HIP warp + MIOpen conv + HIP gates)
      -> decoder -> depth;   state = (h, c), previous depth, previous pose;   "TRACKING LOST" -> reset()

MI355X-specific execution choices (none of them changes results beyond fp32 round-off):
* **feature cache** -- a keyframe's half-resolution features are computed once and reused when the frame later
  serves as a measurement frame (the reference recomputes them, run-testing.py:153-156); eval-mode only;
* **BatchNorm folding** -- conv + eval-mode BN are folded into one biased convolution before inference;
* **epilogue fusion** -- bias add + ReLU / sigmoid after every MIOpen convolution run as one in-place HIP kernel, and
  the 2x bilinear up-sampling of the decoder is a HIP kernel (ATen's takes ~80 us on the 512 x 8 x 10 bottleneck map);
* **no concatenation or state copies** (one sequence per engine, the headline configuration) -- every producer writes straight
  into the buffer its consumer reads: FPN outputs, the cost volume and encoder outputs into channel slices of the encoder's
  concatenation buffers, skip connections and up-sampled maps into the decoder's, the warped hidden state into the ConvLSTM's
  input, the gates into the state buffers in place, the last convolution's epilogue (sigmoid -> depth) into the depth buffer that
  is also next frame's "previous depth"; the FPN's unused 1/32 output is not computed.  ~45 launches per frame less;
* **hipGraph replay** -- after a warm-up frame (MIOpen solver search) the whole frame is captured once per
  (number of measurement frames, has-previous-state) and replayed; the HIP ops are capture-safe (no host sync,
  no allocation inside the C ABI), images and the frame's small matrices live in static device buffers;
* **pose algebra on the host, one upload per frame** -- poses arrive from the host (a tracker, ``poses.txt``); the sweep
  constants and the two relative poses of the frame are evaluated there with the reference's own fp32 expressions
  (``dvmvs.pose_algebra``, default mode "reference": the kernels then sample where the reference samples, bit for bit), packed
  with the intrinsics into one pinned staging slot and sent to the device with a single asynchronous copy ahead of the graph
  launch.  ``pose_algebra="exact"`` evaluates them on the device in fp64 inside the captured frame instead.
"""
import copy
import time
import os

import torch

from dvmvs.config import Config
from dvmvs.hip import ops as _ops
from dvmvs import pose_algebra as _pose_algebra
from dvmvs import utils as _utils
# the engine's parts; the names other code imports from here stay importable from here
from dvmvs.fused_layers import FusedConv2d, _KERNEL_SWITCHES, _graph_microseconds, fold_batchnorm, fuse_epilogues, set_kernel_families      # noqa: F401
from dvmvs.module_surface import GraphedModule, accelerate      # noqa: F401
from dvmvs.frame_host import CopyQueue, FeatureCache, FrameBody
from dvmvs.parameter_block import _MAX_MEAS, ParameterBlock
from dvmvs.frame_direct import DirectFrameBody

# MIOpen's fp32 `igemm_fwd_gtcx35_nhwc_*_gkgs` kernels split the reduction over workgroups and accumulate with float ATOMICS: their
# result differs from run to run (measured: tools/conv_determinism_probe.py -- four layers of a frame, among them 64 -> 64 5x5 at quarter
# resolution), which a depth engine whose recurrent state passes through a discrete z-buffer cannot tolerate (one flipped pixel and the
# runs diverge).  MIOpen reads this switch when it looks for solvers; with the family off it solves those layers with its GEMM /
# Winograd / direct kernels, which are deterministic.  (The bottleneck layers do not reach MIOpen at all: csrc/bottleneck_conv.hip.)
# Set when the PACKAGE is imported (dvmvs/__init__.py: MIOpen reads its MIOPEN_DEBUG_* variables once, at its first convolution, and caches them).
# DepthEngine.__init__ warns when the variable reads differently from what was set there.
import dvmvs as _package
_DETERMINISTIC_MIOPEN = _package.DETERMINISTIC_MIOPEN
_MIOPEN_SWITCH_WAS_PRESET = _package.MIOPEN_SWITCH_WAS_PRESET or os.environ.get("DVMVS_KEEP_MIOPEN_ATOMIC_KERNELS", "0") == "1"

# hipGraphInstantiate gives a graph with two branches an internal stream for the second one, and the hardware queue behind that stream
# alternates from one instantiation to the next (two queues, ROCm 7.2).  Consecutive frames replay the graphs of the two buffer sets: when
# their second branches sit on DIFFERENT queues every frame is 50 us slower (0.855 against 0.805 ms at look-ahead 1, whichever sweep kernel
# runs) -- and which case a run gets used to depend on how many graphs were captured between the two: even (4 sweep configurations per
# buffer set) fast, odd (5, with the MFMA sweep) slow.  So after every two-branch capture this many two-kernel filler graphs are
# instantiated (kept, never launched): all frame graphs end up on the same queue.  DESIGN.md section 5; 0 = the runtime's own order.
_GRAPH_QUEUE_FILLERS = int(os.environ.get("DVMVS_GRAPH_QUEUE_FILLERS", "1"))


def _fork_point(value):
    """A DVMVS_FORK_AFTER value as the fork level of DirectFrameBody._frame_body_direct: -1 ... 4.  Anything else raises -- behind a level the encoder does not have
    the fork would never happen, and the next frame would read features nobody computed."""
    try:
        level = int(value)
    except (TypeError, ValueError):
        level = None
    if level not in (-1, 0, 1, 2, 3, 4):
        raise ValueError(f"DVMVS_FORK_AFTER must be an integer from -1 to 4, got {value!r}")
    return level


_FORK_AFTER = _fork_point(os.environ.get("DVMVS_FORK_AFTER", "1"))      # see DirectFrameBody._frame_body_direct (measured: -1 / 0 / 1 / 2 / 3 / 4 = 1 355 / 1 371 / 1 382 / 1 377 / 1 319 / 1 239 frames/s)


class DepthEngine:
    """Sequential keyframe processor for one video sequence (batch 1: the reference's case) or ``sequences`` = S independent
    sequences advancing in lockstep (batch S: one cost-volume launch, one convolution per layer for all of them), pairnet
    (``lstm_fusion=None``) or fusionnet.

    ``step`` mirrors one iteration of the reference loop; ``reset`` is the "TRACKING LOST" rule (per sequence when S > 1).
    With S > 1 every frame takes the "has a previous frame" path: a sequence without one has zero state, zero previous
    depth and therefore an all-zero depth estimate, for which warp + mask return exactly the zeros the reference's
    first-frame path starts from (convlstm.py:29-41), so the per-sequence results do not depend on what the others do.
    """

    def __init__(self, feature_extractor, feature_shrinker, cost_volume_encoder, lstm_fusion, cost_volume_decoder,
                 device="cuda", min_depth=0.25, max_depth=20.0, n_depth_levels=64, fold_bn=True, cache_features=True,
                 use_graphs=True, cache_size=None, channels_last=False, fuse=True, lstm_channels_last=True, sequences=1,
                 pose_algebra=None, conv_plans=None, bottleneck_convs=None, direct_convs=None, max_lookahead=None, pointwise_convs=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DepthEngine runs on an MI355X; there is no CPU execution path in this package")
        # (before anything is allocated) the encoder halves the frame five times and the decoder doubles its 1/32 map back onto the skip
        # connections: a size that is no multiple of 32 has no 1/32 map whose x2 up-samplings meet the 1/16 ... 1/2 maps
        if Config.test_image_height <= 0 or Config.test_image_width <= 0 or Config.test_image_height % 32 or Config.test_image_width % 32:
            raise ValueError(f"the frame size must be a positive multiple of 32 in both dimensions, got {Config.test_image_width}x{Config.test_image_height} "
                             "(Config.test_image_width x Config.test_image_height)")
        if os.environ.get(_DETERMINISTIC_MIOPEN[0]) != _DETERMINISTIC_MIOPEN[1] and not _MIOPEN_SWITCH_WAS_PRESET:
            import warnings
            warnings.warn(f"{_DETERMINISTIC_MIOPEN[0]} was changed after dvmvs.engine set it: MIOpen may pick atomically accumulating kernels "
                          "and depth is then not bit-reproducible run to run", RuntimeWarning)
        prep = (lambda m: fold_batchnorm(m)) if fold_bn else (lambda m: copy.deepcopy(m).eval())
        mods = [feature_extractor, feature_shrinker, cost_volume_encoder, lstm_fusion, cost_volume_decoder]
        mods = [None if m is None else prep(m).to(self.device) for m in mods]
        if fuse and not channels_last:
            mods = [None if m is None else fuse_epilogues(m) for m in mods]
        if channels_last:
            mods = [None if m is None else m.to(memory_format=torch.channels_last) for m in mods]
        self.fe, self.fs, self.enc, self.lstm, self.dec = mods
        requested = dict(conv_plans=conv_plans, bottleneck_convs=bottleneck_convs, direct_convs=direct_convs, pointwise_convs=pointwise_convs)
        for variable, argument, _ in _KERNEL_SWITCHES:
            wanted = requested[argument] if requested[argument] is not None else os.environ.get(variable, "1") != "0"
            setattr(self, argument, bool(wanted and fuse and not channels_last))
        for m in mods:
            if m is not None:
                set_kernel_families(m, **{argument: getattr(self, argument) for _, argument, _ in _KERNEL_SWITCHES})
        if lstm_channels_last and self.lstm is not None and not channels_last:
            # the ConvLSTM convolution (1024 -> 2048 channels on an 8x10 map, 75 MB of weights) is weight-bandwidth bound;
            # MIOpen's NHWC kernel for it takes 56 us against 88 us for NCHW, which more than pays for the two small layout
            # copies around it (results are those of a different but equally valid fp32 summation order)
            conv = self.lstm.lstm_cell.conv
            conv.weight.data = conv.weight.data.contiguous(memory_format=torch.channels_last)
        self.channels_last = channels_last
        self.min_depth, self.max_depth, self.n_depth_levels = float(min_depth), float(max_depth), int(n_depth_levels)
        self.cache_features = cache_features
        self.cache_size = cache_size or (Config.test_keyframe_buffer_size + 2)
        self.use_graphs = use_graphs
        self.height, self.width = Config.test_image_height, Config.test_image_width
        self.sequences = int(sequences)
        if self.sequences < 1:
            raise ValueError("sequences must be >= 1")
        # destination-passing frame body (see the module docstring): needs the fused epilogues and contiguous channel slices
        self.direct = bool(fuse and fold_bn and not channels_last and self.sequences == 1)
        self.pose_algebra = _pose_algebra._mode(pose_algebra)
        if self.pose_algebra == "auto":      # (the engine takes poses and intrinsics from the host: that is "reference")
            self.pose_algebra = "reference"
        self._prev_pose_host = torch.eye(4).repeat(self.sequences, 1, 1)
        self._no_previous = torch.ones(self.sequences, dtype=torch.bool)   # sequences whose next frame has no previous frame
        self._graphs = {}
        self._static = None
        self._warm = set()
        self.step_clock = None
        self._parity, self._prefetched = 0, None      # buffer set of the next frame; (frame_id, buffer set) whose reference features are ready
        self.plan_frames_ahead = os.environ.get("DVMVS_PLAN_AHEAD", "1") != "0"      # see ParameterBlock.plan_ahead
        self.lookahead_rejected = 0      # announced frames whose prepared stages were not taken because the image came as another tensor
        self._filler_buffers, self._filler_graphs = None, []
        self._copies = CopyQueue()      # open while step() collects its input copies
        self.warm_captured_graphs = os.environ.get("DVMVS_WARM_GRAPHS", "1") != "0"
        # launches of every newly captured graph on throw-away results: the runtime finishes setting a graph up over its first launches (a
        # 5-6 ms device stall was still seen at a graph's third launch, i.e. a few steps into a short run's timed region, with one)
        self.warm_graph_launches = max(1, int(os.environ.get("DVMVS_WARM_GRAPH_LAUNCHES", "3")))
        # how much of the NEXT keyframe a step computes when the caller announces it (step's next_* arguments): 1 its feature extraction,
        # 2 also its sweep + encoder.  Default 1: with the direct convolution kernels the sweep and the encoder fill the chip on their
        # own, and running them next to the decoder only makes both slower (MI355X, 100 steps: level 0 / 1 / 2 = 827 / 1091 / 999
        # frames/s); the feature extractor's small kernels are what overlaps well.  DVMVS_LOOKAHEAD overrides.
        if max_lookahead is None:
            max_lookahead = int(os.environ.get("DVMVS_LOOKAHEAD", "1"))
        self.max_lookahead = max(0, min(2, int(max_lookahead)))
        # what warming up costs (bench.py reports it): wall seconds of the eager first frames, of graph capture, of the first launches of
        # graphs captured ahead; how many such graphs
        self.warmup_seconds = {"eager_first_frames": 0.0, "graph_capture": 0.0, "graph_first_launches": 0.0}
        self.warmup_graphs_launched = 0
        self.sweep_variant_counts = {}     # frames per sweep configuration (dvmvs_cost_volume_fwd's variant) since construction
        # host-planned work list for the sweep: only where the matrices exist on the host, and one plan per launch (one sequence)
        self.sweep_work_list = bool(_utils.SWEEP_WORK_LIST and self.pose_algebra == "reference" and _utils.COST_VOLUME_VARIANT in (0, 2, 3, 4, 5))
        # Round 5: the correlate-then-interpolate sweep (variant 6, csrc/sweep_mfma.hip) takes the keyframe pairs on which its estimated work is
        # small (dvmvs_sweep_plan6: 176 of the sample scene's 285 pairs, 29 us against 33 on the easy ones, 36.5 against 42.0 us over all of them);
        # it reads one 128-byte line per measurement cell, so the engine then keeps its measurement maps -- the feature cache and the per-frame
        # buffers -- channels-last (one transposing launch per keyframe in place of the cache's contiguous copy).  DVMVS_SWEEP_MFMA=0: round 4's
        # all-tiled engine on NCHW maps.
        # (the tiled kernels read channels-last maps only from 64 x 64 cells on -- and so does dvmvs_sweep_plan6 take variant 6)
        self.sweep_mfma = bool(self.direct and self.sweep_work_list and _utils.COST_VOLUME_VARIANT == 0 and os.environ.get("DVMVS_SWEEP_MFMA", "1") != "0"
                               and (self.height // 2) * (self.width // 2) >= 64 * 64)
        # (round 6: dvmvs_sweep_plan6 returns 6 for every single-sequence frame -- one sweep configuration, one frame graph per buffer set and pattern)
        self._tiled_variants = (6,) if self.sweep_mfma else (2, 3, 4, 5)
        self._feature_cache = FeatureCache(self.cache_size, self.device, self.sweep_mfma)
        # the frame's parameter block (host half; its device half comes with the static buffers) and, for one sequence, the destination-passing
        # frame body with its buffer sets (``_direct_buffers``: filled by _allocate_static)
        self._block = ParameterBlock(self.sequences, self.height, self.width, self.n_depth_levels, self.min_depth, self.max_depth, self.pose_algebra,
                                     self.sweep_work_list, self.sweep_mfma, self.is_fusionnet)
        self._frame = DirectFrameBody(*mods, self._block, self.device, self.bottleneck_convs, self.sweep_mfma) if self.direct else None
        self._direct_buffers = self._frame.buffers if self.direct else {}
        self.reset()

    # what the parameter block counts, under the names the engine has always had them (bench.py resets ring_wait_seconds)
    @property
    def ring_wait_seconds(self):
        """Time step() spent waiting for the device at the staging slot (NOT host work: bench.py subtracts it)."""
        return self._block.ring_wait_seconds

    @ring_wait_seconds.setter
    def ring_wait_seconds(self, seconds):
        self._block.ring_wait_seconds = seconds

    @property
    def planned_frames_used(self):
        return self._block.planned_frames_used

    @property
    def _lstm_packed(self):
        """The ConvLSTM convolution's packed weights once the bottleneck kernel has taken it (destination-passing frame body only)."""
        return self._frame._lstm_packed if self.direct else None

    def close(self):
        """Stops the planning thread and puts the interpreter's switch interval back (if DVMVS_SWITCH_INTERVAL made this engine change it)."""
        self._block.close()

    def conv_plan_report(self):
        """[(input shape, weight shape, uses the MIOpen fusion plan, plan us, convolution + epilogue us, max |difference|)] of
        every dense convolution problem timed so far."""
        rows = []
        for m in (self.fe, self.fs, self.enc, self.lstm, self.dec):
            for sub in ([] if m is None else m.modules()):
                if isinstance(sub, FusedConv2d):
                    rows += [(shape, tuple(sub.weight.shape)) + tuple(plan) for shape, plan in sub.plans.items()]
        return rows

    # ---- state ------------------------------------------------------------------------------------------------------
    @property
    def is_fusionnet(self):
        return self.lstm is not None

    def reset(self, sequence=None):
        """Forget the recurrent state and the previous depth/pose (reference: "TRACKING LOST", run-testing.py:97-101), of all
        sequences or of one (S > 1)."""
        if sequence is None or self.sequences == 1:
            self.has_previous = False
            self._no_previous[:] = True
            if self._static is not None:
                for k in ("h", "c", "prev_depth"):
                    self._static[k].zero_()
                if self._direct_buffers:      # the splat's all-zero estimate invariant, also after a frame that failed half-way
                    for buffer_set in self._direct_buffers["sets"]:
                        buffer_set["estimate"].zero_()
        else:
            self._no_previous[sequence] = True
            if self._static is not None:
                for k in ("h", "c", "prev_depth"):
                    self._static[k][sequence].zero_()

    def load_state(self, hidden, cell, previous_depth, previous_pose):
        """Installs a recurrent state (h, c [S,512,H/32,W/32]), previous depth [S,1,H,W] or [S,H,W] and previous pose [S,4,4], e.g. a
        checkpointed one: the next ``step`` continues from it as if this engine had produced it (the state the reference's loop
        carries in lstm_state / previous_depth / previous_pose, fusionnet/run-testing.py:86-88,201-202)."""
        if not self.is_fusionnet:
            raise RuntimeError("pairnet keeps no state between frames")
        self._allocate_static(1)
        s, S = self._static, self.sequences
        s["h"].copy_(hidden.reshape(s["h"].shape))
        s["c"].copy_(cell.reshape(s["c"].shape))
        s["prev_depth"].copy_(previous_depth.reshape(S, 1, self.height, self.width))
        self._prev_pose_host = _pose_algebra.to_host(previous_pose).reshape(S, 4, 4).clone().float()
        self._no_previous[:] = False
        self.has_previous = True

    def state(self):
        """(h, c, previous depth, previous pose) as ``load_state`` takes them (clones; the pose lives on the host)."""
        s = self._static
        return s["h"].clone(), s["c"].clone(), s["prev_depth"].clone(), self._prev_pose_host.clone()

    def clear_feature_cache(self):
        self._feature_cache.clear()

    def new_sequence(self):
        """Start of another video sequence on the same engine: forget the recurrent state AND the cached keyframe features
        (the cache is keyed by the caller's frame ids, which restart with every sequence)."""
        self.reset()
        self.clear_feature_cache()
        self._prefetched = None      # (frame ids restart with the sequence)

    # ---- pieces -----------------------------------------------------------------------------------------------------
    def _features(self, image):
        if self.channels_last:
            image = image.contiguous(memory_format=torch.channels_last)
        return self.fs(*self.fe(image))

    def has_features(self, frame_id):
        """Whether the features of keyframe ``frame_id`` are cached (``step`` then needs no image for it as a measurement frame)."""
        return self.cache_features and frame_id is not None and frame_id in self._feature_cache

    def _half_features(self, frame_id, image):
        if self.has_features(frame_id):
            return self._feature_cache.lookup(frame_id)
        half = self._features(image)[0].contiguous()
        self._remember(frame_id, half)
        return half

    def _remember(self, frame_id, half):
        """Caches a keyframe's half-resolution features (the copy into the cache's buffer rides in the step's copy queue)."""
        if self.cache_features and frame_id is not None:
            self._feature_cache.remember(frame_id, half, self._copies.add)

    def _allocate_static(self, n_meas):
        d, H, W, S = self.device, self.height, self.width, self.sequences
        z = lambda *s: torch.zeros(*s, device=d, dtype=torch.float32)
        if self._static is None:
            block, frame = self._block, self._frame
            block.allocate(d)
            if self.direct:
                frame.allocate()
                direct = frame.buffers
                # the decoder's last concatenation ends with the image; the depth buffer IS next frame's previous depth
                image, depth, ref_half = direct["full_in"][:, 33:36], direct["depth_store"], direct["enc_cat"][0][:, :32]
                state = dict(prev_depth=frame.prev_depth, h=frame.h, c=frame.c, meas_feat=direct["sets"][0]["meas_feat"])
            else:
                image, depth, ref_half = z(S, 3, H, W), z(S, H, W), z(S, 32, H // 2, W // 2)
                state = dict(prev_depth=z(S, 1, H, W), h=z(S, 512, H // 32, W // 32), c=z(S, 512, H // 32, W // 32), meas_feat=[])
            self._static = dict(block.views, image=image, params=block.params, ref_half=ref_half, depth=depth, **state)
        if self.direct:
            self._frame.measurement_buffers(n_meas)
        else:
            while len(self._static["meas_feat"]) < n_meas:
                self._static["meas_feat"].append(z(S, 32, H // 2, W // 2))

    def _frame_body(self, n_meas, has_previous, sweep_variant=0, parity=0, have=0, give=0, n_meas_next=0, next_variant=0):
        """The per-frame computation on the static buffers (this is what gets captured into a hipGraph)."""
        if self.direct:
            # (the fork level is read here, from this module, at every call: bench.py and the tests set it between captures)
            return self._frame._frame_body_direct(n_meas, has_previous, sweep_variant, parity, have, give, n_meas_next, next_variant, fork_after=_FORK_AFTER)
        s = self._static
        feats = self._features(s["image"])
        ref_half = feats[0].contiguous()
        s["ref_half"].copy_(ref_half)
        Hm, kt = self._block.sweep_views(n_meas)
        exact = self.pose_algebra == "exact"
        if exact:
            Hm, kt = _ops.sweep_matrices(s["pose"], s["meas_pose"][:n_meas], s["half_K"])
        cost_volume = _ops.cost_volume(ref_half, s["meas_feat"][:n_meas], Hm, kt, self.min_depth, self.max_depth, self.n_depth_levels,
                                       True, sweep_variant, self._block.sweep_items())
        skip0, skip1, skip2, skip3, bottom = self.enc(ref_half, feats[1], feats[2], feats[3], cost_volume)
        if self.is_fusionnet:
            if has_previous:
                reproject_T = _ops.relative_pose(s["pose"], s["prev_pose"]) if exact else s["reproject_T"]
                lstm_T = _ops.relative_pose(s["prev_pose"], s["pose"]) if exact else s["lstm_T"]
                _, depth_estimation = _ops.depth_reproject_lowres(reproject_T, s["prev_depth"], s["full_K"], s["half_K"], 16)
                state = self.lstm(bottom, (s["h"], s["c"]), s["prev_pose"], s["pose"], depth_estimation, s["lstm_K"], transformation=lstm_T)
            else:
                depth_estimation = torch.zeros(self.sequences, 1, self.height // 32, self.width // 32, device=self.device)
                state = self.lstm(bottom, None, None, s["pose"], depth_estimation, s["lstm_K"])
            s["h"].copy_(state[0])
            s["c"].copy_(state[1])
            bottom = state[0]
        prediction = self.dec(s["image"], skip0, skip1, skip2, skip3, bottom, full_resolution_only=True)[0]
        s["depth"].copy_(prediction)
        if self.is_fusionnet:
            s["prev_depth"].copy_(prediction.view(self.sequences, 1, self.height, self.width))

    # ---- public -----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, reference_image, reference_pose, measurement_images, measurement_poses, full_K, frame_id=None,
             measurement_ids=None, next_reference_image=None, next_frame_id=None, next_reference_pose=None,
             next_measurement_poses=None, next_measurement_ids=None):
        """One keyframe (of each of the S sequences).  Images [S,3,H,W] normalised, on the GPU; poses [S,4,4] cam-to-world and
        ``full_K`` [S,3,3] preferably as HOST tensors (that is where they come from, and where the frame's small matrices are
        evaluated; device tensors are copied back, which synchronises).  With S > 1 the sequences advance in lockstep:
        ``frame_id`` / ``measurement_ids`` name the step for all of them and a cached feature entry holds all S maps.

        ``measurement_images[i]`` may be ``None`` when ``measurement_ids[i]`` is in the feature cache.

        Look-ahead (one sequence per engine), for callers that already know the NEXT call's frame -- a pre-computed keyframe index, a
        camera that is a frame ahead.  The stages of a frame that carry no recurrent state are computed for the next frame during
        THIS call, on a second stream, concurrently with this frame's ConvLSTM and decoder:
        * ``next_reference_image`` + ``next_frame_id``: its MnasNet + FPN features;
        * additionally ``next_reference_pose``, ``next_measurement_poses`` and ``next_measurement_ids`` (every one of them this call's
          ``frame_id`` or a cached keyframe): its plane sweep and cost-volume encoder as well.
        The next call (same ``frame_id``; same poses / measurement ids for the second level) finds them ready; anything else is simply
        recomputed.  Same kernels on the same inputs: results are bit-identical to calls without look-ahead.
        Returns the full-resolution depth [S,H,W] (a static buffer that the next call overwrites: clone to keep).
        """
        n_meas = len(measurement_poses)
        if n_meas < 1 or n_meas > _MAX_MEAS:
            raise ValueError(f"need between 1 and {_MAX_MEAS} measurement frames")
        measurement_ids = measurement_ids or [None] * n_meas
        clock = self.step_clock      # None, or a list that receives this step's host checkpoints (tools/step_times_probe.py)
        if clock is not None:
            marks = [("enter", time.perf_counter())]
            clock.append(marks)
            mark = lambda name: marks.append((name, time.perf_counter()))
        else:
            mark = lambda name: None
        self._allocate_static(n_meas)
        s = self._static
        if tuple(reference_image.shape) != (self.sequences, 3, self.height, self.width):
            raise ValueError(f"image must be [{self.sequences},3,{self.height},{self.width}], got {tuple(reference_image.shape)}")
        parity = self._parity if self.direct else 0
        cur = self._direct_buffers["sets"][parity] if self.direct else None
        announced = dict(image=next_reference_image, frame_id=next_frame_id, pose=next_reference_pose, measurement_poses=next_measurement_poses,
                         measurement_ids=next_measurement_ids)
        self._copies.open()      # (closed at "inputs copied"; an exception on the way issues what was queued: see the except clause there)
        try:
            if self.direct:
                self._direct_buffers["estimate"] = cur["estimate"]      # (diagnostics: the 8x10 depth estimate of the frame this call computes)
            have = self._prepared_level(frame_id, parity, reference_image, reference_pose, measurement_ids, measurement_poses, full_K)
            if have >= 1 and self.cache_features:
                self._remember(frame_id, cur["ref_half_nhwc"] if self.sweep_mfma else cur["enc_cat"][0][:, :32])     # (the next frame may use this one as a measurement frame)
            if have < 2:      # (its measurement features are not needed when its sweep already ran)
                self._queue_measurement_features(cur["meas_feat"] if self.direct else s["meas_feat"], n_meas, measurement_images, measurement_ids)
            give, next_frame = self._plan_next_frame(announced, reference_image, frame_id, parity, have)
            self._queue_images(cur, parity, have, give, reference_image, next_reference_image)
        except BaseException:
            CopyQueue.issue(self._copies.close())      # (what was queued belongs to cache entries that are already registered: write it before the error leaves)
            raise
        pending = self._copies.close()      # (launched together with the parameter block: ParameterBlock.upload)
        mark("inputs copied")
        committed_pose, sweep_variant, next_variant = self._block.upload(n_meas, reference_pose, measurement_poses, full_K, self._prev_pose_host, self._no_previous,
                                                                         index=parity, own_sweep=have < 2, next_frame=next_frame, pending_copies=pending)
        mark("parameters planned + uploaded")
        if self.direct and give < 2 and self.pose_algebra == "reference" and self.plan_frames_ahead and next_reference_pose is not None and \
                next_measurement_poses is not None and 1 <= len(next_measurement_poses) <= _MAX_MEAS:
            # the announced next frame's parameter block, evaluated on the planning thread while this thread launches the frame
            self._block.plan_ahead(len(next_measurement_poses), next_reference_pose, list(next_measurement_poses), full_K, committed_pose, 1 - parity)
        if have == 2:
            sweep_variant = self._prefetched["sweep_variant"]
        self.sweep_variant_counts[sweep_variant] = self.sweep_variant_counts.get(sweep_variant, 0) + 1
        # S > 1: always the previous-state path (see the class docstring); S == 1: the reference's two frame kinds
        body = FrameBody(n_meas, (self.has_previous or self.sequences > 1) and self.is_fusionnet, sweep_variant, parity, have, give,
                         len(next_frame[1]) if next_frame else 0, next_variant or 0)
        self._launch(body, cur)
        mark("frame launched")
        self._commit(committed_pose, frame_id, cur, parity, have, give, next_variant, announced, full_K)
        mark("done")
        return s["depth"]

    # ---- the parts of a step, in its order ---------------------------------------------------------------------------------
    @staticmethod
    def _is_announced_tensor(ready, image):
        """Whether ``image`` is the very tensor that ``ready`` (a ``_prefetched`` record) was prepared from: same storage, unmodified since (its
        ``_version``), same device, same strides.  A frame id alone does not identify an image; the engine keeps the announced tensor alive, so
        the address cannot have been reused."""
        return (ready["image"].data_ptr() == image.data_ptr() and ready["image_version"] == image._version and
                ready["image"].device == image.device and tuple(ready["image"].stride()) == tuple(image.stride()))

    def _prepared_level(self, frame_id, parity, reference_image, reference_pose, measurement_ids, measurement_poses, full_K):
        """What the previous call prepared for this frame: 0 nothing, 1 its reference features, 2 also its sweep + encoder."""
        ready = self._prefetched
        if not self.direct or ready is None or frame_id is None or ready["frame_id"] != frame_id or ready["parity"] != parity:
            return 0
        if not self._is_announced_tensor(ready, reference_image):
            # the announced frame came as ANOTHER tensor (re-materialised, modified): its prepared stages are not taken (say so)
            self.lookahead_rejected += 1
            if self.lookahead_rejected == 1:
                import warnings
                warnings.warn("DepthEngine.step: the frame announced by next_reference_image arrived as a different (or modified) tensor; its "
                              "prepared features are recomputed.  Hand step() the very tensor that was announced to keep the look-ahead.", RuntimeWarning)
            return 0
        to_host = _pose_algebra.to_host
        if ready["level"] == 2 and ready["measurement_ids"] == list(measurement_ids) and len(ready["measurement_poses"]) == len(measurement_poses) and \
                torch.equal(ready["full_K"], to_host(full_K).reshape(-1, 3, 3)) and torch.equal(ready["pose"], to_host(reference_pose).reshape(-1, 4, 4)) and \
                all(torch.equal(a, to_host(b).reshape(-1, 4, 4)) for a, b in zip(ready["measurement_poses"], measurement_poses)):
            return 2
        return 1

    def _queue_measurement_features(self, target, n_meas, measurement_images, measurement_ids):
        """This frame's measurement features, out of the cache or computed, into the sweep's buffers ``target``."""
        # resolve every measurement frame BEFORE anything is inserted into the cache: an insertion may evict the least
        # recently used entry, which could be a frame this very call still needs
        fresh = []
        for i in range(n_meas):
            img = measurement_images[i] if measurement_images is not None else None
            mid = measurement_ids[i]
            if self.has_features(mid):
                half = self._feature_cache.lookup(mid)
            elif img is None:
                raise ValueError(f"measurement frame {mid} is not cached and no image was given")
            else:
                half = self._features(img)[0].contiguous()
                fresh.append((mid, half))
            self._copies.add(target[i], half)
        for mid, half in fresh:
            self._remember(mid, half)

    def _plan_next_frame(self, announced, reference_image, frame_id, parity, have):
        """How much of the announced next frame this call computes: (0 nothing / 1 its features / 2 also its sweep + encoder, (pose, measurement
        poses) of a frame whose sweep runs now -- its measurement features are queued into the other buffer set -- or None)."""
        if not self.direct or announced["image"] is None or self.max_lookahead < 1:
            return 0, None
        if tuple(announced["image"].shape) != tuple(reference_image.shape):
            raise ValueError("next_reference_image must have the reference image's shape")
        poses, ids = announced["measurement_poses"], announced["measurement_ids"]
        if not (self.max_lookahead >= 2 and announced["pose"] is not None and poses is not None and ids is not None and
                announced["frame_id"] is not None and self.pose_algebra == "reference" and self.cache_features and
                1 <= len(poses) <= _MAX_MEAS and len(ids) == len(poses) and
                all(m is not None and (m in self._feature_cache or (m == frame_id and have >= 1)) for m in ids)):
            return 1, None
        self._allocate_static(len(poses))
        for i, mid in enumerate(ids):
            self._copies.add(self._direct_buffers["sets"][1 - parity]["meas_feat"][i], self._feature_cache[mid])
        return 2, (announced["pose"], list(poses))

    def _queue_images(self, cur, parity, have, give, reference_image, next_reference_image):
        """The images into their homes (the decoder's last concatenation buffer ends with the image)."""
        s = self._static
        if self.direct:
            if have < 1:
                self._copies.add(cur["full_in"][:, 33:36], reference_image)
            if give >= 1:
                self._copies.add(self._direct_buffers["sets"][1 - parity]["full_in"][:, 33:36], next_reference_image)
            s["image"], s["ref_half"] = cur["full_in"][:, 33:36], cur["enc_cat"][0][:, :32]
        else:
            self._copies.add(s["image"], reference_image)

    def _launch(self, body, cur):
        """Runs the frame ``body``: eagerly (no graphs, or the first frame of its kind), else by replaying its graph -- with everything this kind of
        frame will need later captured and warmed first when the graph is new."""
        kind = (body.n_meas, body.has_previous)
        if not self.use_graphs:
            self._frame_body(*body)
        elif kind not in self._warm:
            # first occurrence of this kind of frame: run eagerly (lets MIOpen pick its solvers, times the fusion plans); state
            # buffers are updated by the body, so this is a real frame, not a throw-away
            t_eager = time.perf_counter()
            self._frame_body(*body)
            self._warm.add(kind)
            torch.cuda.synchronize(self.device)
            self.warmup_seconds["eager_first_frames"] += time.perf_counter() - t_eager
        else:
            key, known = body.key(), len(self._graphs)
            if key not in self._graphs:
                self._capture_ahead(body)
                if self.warm_captured_graphs:      # (the graph of THIS frame is warmed like the ones captured ahead: its throw-away launches are undone the same way)
                    self._warm_graphs(list(self._graphs)[known:], cur, body.have)      # (a dict keeps the order of insertion: the new ones)
            self._graphs[key].replay()

    def _capture_ahead(self, body):
        """Captures the graph of ``body`` and, behind it, those this kind of frame will need later.  Capture records launches, it executes nothing
        -- so they are captured now, while the caller is still warming up: with look-ahead the steady-state pattern (this frame's share
        prefetched, the next frame's being prefetched) for both buffer sets and both sweep configurations, without it both configurations.  A
        later frame whose geometry asks for the other configuration finds its graph ready instead of paying ~0.1 s of capture mid-run."""
        def capture(b):
            if b.key() not in self._graphs:
                self._graphs[b.key()] = self._capture(b)

        t_capture = time.perf_counter()
        capture(body)
        give, tiled = body.give, self._tiled_variants
        if give:
            # the sweep's configurations x (two passes, one pass) [+ the MFMA sweep]: whichever a later geometry asks for
            choices = tiled if body.next_variant in tiled or body.sweep_variant in tiled else (body.sweep_variant,)
            for par in (0, 1):
                for v in (choices if give < 2 else (0,)):
                    for vn in (choices if give == 2 else (0,)):
                        capture(body._replace(sweep_variant=v, parity=par, have=give, next_variant=vn))
        elif body.sweep_variant in tiled and body.have < 2:
            for par in ((0, 1) if self.direct else (0,)):
                for v in tiled:
                    capture(body._replace(sweep_variant=v, parity=par))
        self.warmup_seconds["graph_capture"] += time.perf_counter() - t_capture

    def _warm_graphs(self, fresh, cur, have):
        """Launches the newly captured graphs ``fresh`` on throw-away results and puts the state back.  A graph's FIRST launch stalls the device
        for ~5 ms (its kernel arguments and code are set up then, not at capture): once per pre-captured graph, i.e. a few steps into every
        run, whenever a geometry first asks for another sweep configuration or buffer set.  So every graph captured ahead is launched now,
        during warm-up: the recurrent state is put back afterwards, and everything else the launch writes is rewritten by the real frame
        (same image, same features) before anybody reads it.
        One exception: a frame whose sweep + encoder ran a frame ahead (have == 2) does NOT recompute them, and a fresh graph of the other
        parity runs ITS look-ahead stage -- other measurement count, other sweep configuration, the work list of another geometry -- on this
        frame's buffer set ``cur``.  Those buffers are saved and put back as well."""
        t_warm = time.perf_counter()
        s = self._static
        keep = [(s[k], s[k].clone()) for k in ("h", "c", "prev_depth")] if self.is_fusionnet else []
        keep += [(t, t.clone()) for t in self._tensors(cur)] if (self.direct and have == 2) else []
        for k in fresh:      # back to back per graph: a graph's next launch is queued while its previous one still runs, as in the steady
            for _ in range(self.warm_graph_launches):      # state, where the host is up to two frames ahead of the device
                self._graphs[k].replay()
        for tensor, saved in keep:
            tensor.copy_(saved)
        if self.direct:      # (the splat's invariant: a frame finds its estimate buffer all-zero; the throw-away launches wrote into both)
            for buffer_set in self._direct_buffers["sets"]:
                buffer_set["estimate"].zero_()
        torch.cuda.synchronize(self.device)
        self.warmup_seconds["graph_first_launches"] += time.perf_counter() - t_warm
        self.warmup_graphs_launched += len(fresh)

    def _commit(self, committed_pose, frame_id, cur, parity, have, give, next_variant, announced, full_K):
        """The launched frame becomes "the previous frame" (only now: a frame that raised has left the state that of one frame), what was
        announced and computed ahead is recorded for the next call, and the frame's features go into the cache."""
        self._prev_pose_host = committed_pose
        self._no_previous[:] = False
        self.has_previous = True
        if self.direct:
            self._prefetched = None
            if give >= 1 and announced["frame_id"] is not None:
                self._prefetched = dict(frame_id=announced["frame_id"], parity=1 - parity, level=give, sweep_variant=next_variant,
                                        image=announced["image"], image_version=announced["image"]._version)
                if give == 2:
                    to_host = _pose_algebra.to_host
                    self._prefetched.update(pose=to_host(announced["pose"]).reshape(-1, 4, 4).clone(), measurement_ids=list(announced["measurement_ids"]),
                                            full_K=to_host(full_K).reshape(-1, 3, 3).clone(),      # (the sweep ahead used THIS call's intrinsics)
                                            measurement_poses=[to_host(p).reshape(-1, 4, 4).clone() for p in announced["measurement_poses"]])
            self._parity = 1 - parity
        if self.cache_features and frame_id is not None and have < 1:
            self._remember(frame_id, cur["ref_half_nhwc"] if (self.direct and self.sweep_mfma) else self._static["ref_half"])

    @staticmethod
    def _tensors(tree):
        """Every tensor of a (nested dict / list of) buffer set, in a fixed order."""
        if isinstance(tree, torch.Tensor):
            return [tree]
        values = tree.values() if isinstance(tree, dict) else tree if isinstance(tree, (list, tuple)) else ()
        return [t for v in values for t in DepthEngine._tensors(v)]

    def graph_memory_report(self):
        """Captured frame graphs and the device memory of their private pools (bytes; None where the runtime does not say)."""
        pools = None
        try:
            stats = torch.cuda.memory_stats(self.device)
            pools = int(stats.get("reserved_bytes.all.current", 0)) - int(stats.get("allocated_bytes.all.current", 0))
        except Exception:
            pass
        return {"graphs": len(self._graphs), "graphs_launched_once_at_warmup": self.warmup_graphs_launched, "queue_filler_graphs": len(self._filler_graphs),
                "reserved_minus_allocated_bytes": pools, "warmup_seconds": {k: round(v, 4) for k, v in self.warmup_seconds.items()}}

    def refresh_weights(self):
        """Call after loading new parameters into this engine's modules (``engine.fe`` ... ``engine.dec``): the MFMA convolution kernels
        read re-packed copies of the weights, made at first use.  They are re-packed IN PLACE, so captured graphs stay valid."""
        for m in (self.fe, self.fs, self.enc, self.lstm, self.dec):
            for sub in ([] if m is None else m.modules()):
                if isinstance(sub, FusedConv2d):
                    sub.repack()
        if self.direct:
            self._frame.repack()

    def _capture(self, body):
        """Captures the frame body ``body`` (a FrameBody) into a hipGraph.  Capture only records the launches (nothing executes, no
        state buffer changes); the caller replays the graph to actually run the frame."""
        torch.cuda.synchronize(self.device)
        graph = torch.cuda.CUDAGraph()
        if getattr(self, "graph_debug", False):     # bench.py counts the kernel nodes of the frame graph from its dot dump
            graph.enable_debug_mode()
        with torch.cuda.graph(graph):
            self._frame_body(*body)
        if self.direct and body.give and body.have >= body.give:      # a body with a second branch (see _frame_body_direct)
            for _ in range(_GRAPH_QUEUE_FILLERS):
                self._capture_queue_filler()
        return graph

    def _capture_queue_filler(self):
        """A two-branch graph of two tiny kernels, instantiated and never launched (see _GRAPH_QUEUE_FILLERS)."""
        if self._filler_buffers is None:
            self._filler_buffers = torch.zeros(2, 64, device=self.device)
        filler = torch.cuda.CUDAGraph()
        with torch.cuda.graph(filler):
            main = torch.cuda.current_stream(self.device)
            side = self._frame.side_stream
            side.wait_stream(main)
            with torch.cuda.stream(side):
                self._filler_buffers[0].add_(1.0)
            self._filler_buffers[1].add_(1.0)
            main.wait_stream(side)
        self._filler_graphs.append(filler)

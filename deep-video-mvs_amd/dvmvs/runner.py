"""Scene runners: the loops of the reference's run-testing.py (pre-computed keyframe index) and run-testing-online.py
(KeyframeBuffer on the fly) around the MI355X frame engine.

/root/reference/dvmvs/fusionnet/run-testing.py:67-230 and run-testing-online.py:71-232, without cv2 / path / tqdm.  A scene
folder holds ``images/*.png``, ``poses.txt`` (one 4x4 camera-to-world per line), ``K.txt`` and optionally ``depth/*.png``
(uint16 millimetres).  Both runners return (predictions, reference_depths or None, InferenceTimer); ``save_results`` from
``dvmvs.utils`` writes the same ``.npz`` files as the reference.
"""
import os

import numpy as np
import torch

from dvmvs.config import Config
from dvmvs.dataset_loader import (FrameUploader, PreprocessImage, load_depth_png, load_depth_png_u16, load_image, load_image_u8,
                                  resize_nearest)
from dvmvs.engine import DepthEngine
from dvmvs.keyframe_buffer import KeyframeBuffer
from dvmvs.utils import InferenceTimer

SCALE_RGB = 255.0
MEAN_RGB = [0.485, 0.456, 0.406]
STD_RGB = [0.229, 0.224, 0.225]


class Scene:
    """``raw=True``: ``image`` / ``depth`` return the files as decoded (uint8 RGB, uint16 millimetres) for pre-processing on the device."""

    def __init__(self, folder, raw=False):
        self.folder = str(folder)
        self.raw = bool(raw)
        self.K = np.loadtxt(os.path.join(self.folder, "K.txt")).astype(np.float32)
        self.poses = np.fromfile(os.path.join(self.folder, "poses.txt"), dtype=float, sep="\n ").reshape((-1, 4, 4))
        self.image_names = sorted(n for n in os.listdir(os.path.join(self.folder, "images")) if n.endswith(".png"))
        depth_dir = os.path.join(self.folder, "depth")
        self.depth_names = sorted(n for n in os.listdir(depth_dir) if n.endswith(".png")) if os.path.isdir(depth_dir) else None

    def image(self, i):
        return (load_image_u8 if self.raw else load_image)(os.path.join(self.folder, "images", self.image_names[i]))

    def depth(self, i):
        return (load_depth_png_u16 if self.raw else load_depth_png)(os.path.join(self.folder, "depth", self.depth_names[i]))

    def pose(self, i):
        """[1,4,4] float32 on the host (poses and K stay there: DepthEngine.step)."""
        return torch.from_numpy(self.poses[i]).float().unsqueeze(0)


def _to_device(image_hwc, device):
    return torch.from_numpy(np.ascontiguousarray(np.transpose(image_hwc, (2, 0, 1)))).float().unsqueeze(0).to(device)


def _preprocessor(scene, raw_image, size=None, crop=None):
    """The PreprocessImage of a raw frame of ``scene``: the one place a scene run builds it.  ``size`` = (width, height) and ``crop`` =
    (distortion_crop, perform_crop) default to the fusionnet's (Config.test_*)."""
    width, height = size or (Config.test_image_width, Config.test_image_height)
    distortion_crop, perform_crop = crop or (Config.test_distortion_crop, Config.test_perform_crop)
    return PreprocessImage(K=scene.K, old_width=raw_image.shape[1], old_height=raw_image.shape[0], new_width=width, new_height=height,
                           distortion_crop=distortion_crop, perform_crop=perform_crop)


class FrameInput:
    """The frames of one scene run as network inputs: opens the scene and, with ``device_preprocess``, owns the FrameUploader.  ``rgb`` =
    (scale, mean, std); ``size`` and ``crop`` as in ``_preprocessor``.  ``ahead`` holds an image that was prepared before its turn (the
    offline fusionnet loop's look-ahead), by frame index."""

    def __init__(self, scene_folder, device, device_preprocess, rgb=(SCALE_RGB, MEAN_RGB, STD_RGB), size=None, crop=None):
        self.scene = Scene(scene_folder, raw=device_preprocess)
        self.device, self.rgb, self.size, self.crop = torch.device(device), rgb, size, crop
        self.uploader = FrameUploader(self.device) if device_preprocess else None
        self.ahead = {}

    def preprocessor(self, raw):
        return _preprocessor(self.scene, raw, self.size, self.crop)

    def prepare(self, pre, raw):
        """Network input [1,3,h,w] on the device: on the host (numpy, then a blocking copy) or, with ``device_preprocess``, from the raw 8-bit
        frame in one kernel launch behind a pinned, non-blocking copy."""
        if self.uploader is None:
            return _to_device(pre.apply_rgb(raw, *self.rgb), self.device)
        return pre.apply_rgb_device(raw, *self.rgb, device=self.device, uploader=self.uploader)

    def image(self, pre, index):
        return self.prepare(pre, self.scene.image(index))

    @staticmethod
    def intrinsics(pre):
        return torch.from_numpy(pre.get_updated_intrinsics()).float().unsqueeze(0)


class KeyframeIndex:
    """A keyframe index file ("ref meas1 meas2 ..." or "TRACKING LOST" per line), cut to ``max_frames`` lines and then parsed: ``lines``
    (stripped, for ``frame_log``), ``frames`` (per line the frame positions [ref, meas1, ...], or None where tracking was lost),
    ``next_keyframe`` (per line the number of the next line that is not a tracking loss, or None) and ``n_predictions``."""

    def __init__(self, keyframe_index_file, image_names, max_frames=None):
        position = {name: i for i, name in enumerate(image_names)}
        with open(keyframe_index_file) as f:
            self.lines = [l.strip() for l in f if l.strip()][:max_frames]
        self.frames = [None if line == "TRACKING LOST" else [position[name] for name in line.split(" ")] for line in self.lines]
        self.n_predictions = sum(frames is not None for frames in self.frames)
        self.next_keyframe, upcoming = [None] * len(self.lines), None
        for n in reversed(range(len(self.lines))):
            self.next_keyframe[n] = upcoming
            if self.frames[n] is not None:
                upcoming = n

    def __iter__(self):
        """(line, its frames or None, the next keyframe's frames or None) per line."""
        for line, frames, upcoming in zip(self.lines, self.frames, self.next_keyframe):
            yield line, frames, (self.frames[upcoming] if upcoming is not None else None)


class DeviceEvaluation:
    """Predictions, ground-truth depths and their error metrics kept on the device while a scene runs (``device_evaluate=True``), so that
    no frame waits for a transfer: per prediction a slot of a pre-sized block -- the prediction copied device-to-device on the current
    stream (the engine's output buffer is static: the next frame overwrites it), the ground truth next to it, and one
    dvmvs.hip.ops.depth_errors launch that writes the frame's row of the block's metric table (max_depth = inf, save_results' default).
    A block is ONE float32 buffer (predictions, ground truths, table), fetched with one copy by ``finish``; a runner that does not know
    its number of predictions in advance gets further blocks of ``capacity`` slots as it goes.  The ground truth is either written into
    its slot by the device pre-processing (``slot.gt`` as ``out=``) or, when it was pre-processed on the host, sent through a pinned
    staging ring (``stage``: float32 on the device for the metrics; the host array itself is what ``finish`` returns)."""

    class Slot:
        def __init__(self, block, index):
            self.pred, self.row = block["preds"][index], block["table"][index:index + 1]
            self.gt = block["gts"][index] if block["gts"] is not None else None
            self.staged = None

    def __init__(self, device, with_depth, gt_on_device, capacity):
        self.device = torch.device(device)
        self.with_depth, self.gt_on_device, self.capacity = bool(with_depth), bool(gt_on_device), max(int(capacity), 1)
        self.blocks, self.count, self.host_gts = [], 0, []
        self.stager = FrameUploader(self.device) if self.with_depth and not self.gt_on_device else None

    def next_slot(self, height, width):
        index = self.count % self.capacity
        if index == 0:
            frame, n = height * width, self.capacity
            maps = 2 if self.with_depth and self.gt_on_device else 1
            buffer = torch.empty(n * (maps * frame + 8), dtype=torch.float32, device=self.device)
            self.blocks.append({"buffer": buffer, "frame": frame, "shape": (height, width), "maps": maps,
                                "preds": buffer[:n * frame].view(n, height, width),
                                "gts": buffer[n * frame:2 * n * frame].view(n, height, width) if maps == 2 else None,
                                "table": buffer[maps * n * frame:].view(n, 8)})
        block = self.blocks[-1]
        if block["shape"] != (height, width):
            raise ValueError(f"device evaluation: a {height}x{width} frame in a scene of {block['shape'][0]}x{block['shape'][1]} frames")
        return DeviceEvaluation.Slot(block, index)

    def stage(self, slot, host_depth):
        """Ground truth pre-processed on the host: kept as it is for the caller, and sent (as float32, without a blocking copy) for the metrics."""
        self.host_gts.append(host_depth)
        flat = self.stager.upload(np.ascontiguousarray(host_depth, dtype=np.float32))
        slot.staged = flat.view(torch.float32).view(tuple(host_depth.shape))

    def commit(self, slot, depth):
        from dvmvs.hip import ops
        slot.pred.copy_(depth.reshape(slot.pred.shape), non_blocking=True)
        if self.with_depth:
            ops.depth_errors(slot.staged if slot.staged is not None else slot.gt, slot.pred, out=slot.row)
        self.count += 1

    def finish(self, error_log=None):
        """(predictions, ground truths or None) as lists of numpy arrays; ``error_log`` receives the float32 [8] rows.  One download per block."""
        predictions, gts, left = [], [], self.count
        for block in self.blocks:
            n, used = self.capacity, min(left, self.capacity)
            left -= used
            host = block["buffer"].cpu().numpy()
            frame, shape, maps = block["frame"], block["shape"], block["maps"]
            predictions.extend(host[:n * frame].reshape((n,) + shape)[:used])
            if maps == 2:
                gts.extend(host[n * frame:2 * n * frame].reshape((n,) + shape)[:used])
            if self.with_depth and error_log is not None:
                error_log.extend(host[maps * n * frame:].reshape(n, 8)[:used].copy())
        if not self.with_depth:
            return predictions, None
        return predictions, (gts if self.gt_on_device else self.host_gts)


class SceneResults:
    """What a scene run returns, by one of three routes chosen here: the host route (the prediction is fetched per frame, the ground truth
    pre-processed with numpy), ``device_preprocess`` alone (the ground truth is pre-processed on the device and fetched together with the
    prediction) and ``device_evaluate`` (a DeviceEvaluation: nothing is fetched before ``finish``).  ``frames``: the run's FrameInput
    (scene, device, uploader); ``capacity``: the number of predictions, or the block size where it is not known.
    ``fuse``: a ``dvmvs.tsdf.LiveFusion`` (or None): every prediction is also handed to ``fuse.add`` where it lies on the device, with the
    inputs ``dvmvs.tsdf.run`` would read back from files -- the pre-processor's updated intrinsics, the frame's pose as float32 and the
    frame's colour resized (nearest) to the prediction size as 8-bit.  ``add`` enqueues and returns: no route waits longer for it."""

    def __init__(self, frames, evaluate, device_evaluate, capacity, error_log=None, fuse=None):
        self.frames, self.error_log, self.fuse = frames, error_log, fuse
        self.want_depth = bool(evaluate and frames.scene.depth_names)
        self.evaluation = None
        if device_evaluate:
            self.evaluation = DeviceEvaluation(frames.device, self.want_depth, frames.uploader is not None, capacity)
        self.predictions, self.reference_depths = [], []

    def begin(self, pre, reference_index, raw=None):
        """Before the timed region: enqueues the ground truth of the frame (``pre``: its PreprocessImage) where the route has it on the device.
        ``raw``: the frame as the scene decoded it, when the caller has it (used by ``fuse`` only: no image is decoded twice)."""
        scene, device, uploader = self.frames.scene, self.frames.device, self.frames.uploader
        self.pre, self.reference_index, self.slot, self.depth_on_device = pre, reference_index, None, None
        if self.fuse is not None:       # the colour dvmvs.tsdf.run integrates: crop window (if any), nearest resize, 8 bits
            raw = scene.image(reference_index) if raw is None else raw
            self.fuse_colour = np.ascontiguousarray(resize_nearest(pre._crop(raw) if pre.perform_crop else raw, pre.new_width,
                                                                   pre.new_height).astype(np.uint8))
        if self.evaluation is not None:
            self.slot = self.evaluation.next_slot(pre.new_height, pre.new_width)
            if self.want_depth and uploader is not None:
                pre.apply_depth_device(scene.depth(reference_index), device=device, uploader=uploader, out=self.slot.gt.unsqueeze(0))
            elif self.want_depth:
                self.evaluation.stage(self.slot, pre.apply_depth(scene.depth(reference_index)))
        elif self.want_depth and uploader is not None:
            self.depth_on_device = pre.apply_depth_device(scene.depth(reference_index), device=device, uploader=uploader)

    def add(self, depth):
        """After the timed region: the network's depth [1,1,h,w] (a static buffer is fine: it is copied or fetched here)."""
        if self.fuse is not None:
            self.fuse.add(depth, self.fuse_colour, self.pre.get_updated_intrinsics(),
                          self.frames.scene.poses[self.reference_index].astype(np.float32))
        if self.evaluation is not None:              # prediction, ground truth and metrics stay on the device: nothing waits here
            self.evaluation.commit(self.slot, depth)
            return
        if self.depth_on_device is not None:         # one transfer for both maps (same size: the network's)
            prediction, reference_depth = torch.stack((depth.reshape(self.depth_on_device.shape[-2:]), self.depth_on_device[0])).cpu().numpy()
        else:
            prediction = depth.cpu().numpy().squeeze()
            reference_depth = self.pre.apply_depth(self.frames.scene.depth(self.reference_index)) if self.want_depth else None
        self.predictions.append(prediction)
        self.reference_depths.append(reference_depth)

    def finish(self, timer):
        """(predictions, reference depths or None, timer); ``device_evaluate``: one download, the rows into ``error_log``, the timer resolved."""
        if self.evaluation is not None:
            predictions, reference_depths = self.evaluation.finish(self.error_log)
            timer.resolve()
            return predictions, reference_depths, timer
        return self.predictions, (self.reference_depths if self.want_depth else None), timer


def _run_frame(engine, frames, results, timer, indices, upcoming=None):
    """One prediction: ``indices`` = [reference, measurement, ...] frame positions.  ``upcoming``: the same of the NEXT call when it is known
    (offline runs): its reference image is pre-processed now and handed to the engine as look-ahead (DepthEngine.step: its features, sweep
    and encoder run concurrently with this frame), and kept in ``frames.ahead`` for that next call."""
    scene = frames.scene
    reference_index, measurement_indices = indices[0], indices[1:]
    raw = scene.image(reference_index)
    pre = frames.preprocessor(raw)
    ref_image = frames.ahead.pop(reference_index, None)
    if ref_image is None:
        ref_image = frames.prepare(pre, raw)
    next_image = None
    if upcoming is not None:
        raw_next = scene.image(upcoming[0])
        next_image = frames.prepare(frames.preprocessor(raw_next), raw_next)
        frames.ahead = {upcoming[0]: next_image}
    ref_pose, full_K = scene.pose(reference_index), FrameInput.intrinsics(pre)
    meas_images, meas_poses = [], []
    for m in measurement_indices:
        if engine.cache_features and engine.has_features(m):
            meas_images.append(None)     # features of this keyframe are cached: no need to load / pre-process the image again
        else:
            meas_images.append(frames.image(pre, m))
        meas_poses.append(scene.pose(m))
    results.begin(pre, reference_index, raw=raw)
    timer.record_start_time()
    ahead = {}
    if upcoming is not None:      # the next reference image and its poses: the engine then also runs its sweep + encoder a frame ahead
        ahead = dict(next_reference_image=next_image, next_frame_id=upcoming[0], next_reference_pose=scene.pose(upcoming[0]),
                     next_measurement_poses=[scene.pose(m) for m in upcoming[1:]], next_measurement_ids=list(upcoming[1:]))
    depth = engine.step(ref_image, ref_pose, meas_images, meas_poses, full_K, frame_id=reference_index,
                        measurement_ids=list(measurement_indices), **ahead)
    timer.record_end_time_and_elapsed_time()
    results.add(depth)


def predict_offline(engine: DepthEngine, scene_folder, keyframe_index_file, evaluate=True, max_frames=None, frame_log=None,
                    device_preprocess=False, device_evaluate=False, error_log=None, fuse=None):
    """Runs the lines of a keyframe index file ("ref meas1 meas2 ..." or "TRACKING LOST") through ``engine``.
    ``frame_log`` (a list) receives the line each prediction belongs to: "ref meas1 ..." file names, or "TRACKING LOST".
    ``device_preprocess``: frames are loaded as 8-bit images, uploaded through a ring of pinned buffers and cropped / resized / normalised
    by one kernel launch each (dvmvs.hip.ops.preprocess_rgb; the ground-truth depth likewise, returned as float32) instead of by numpy
    on the host.  Default False: the host path, unchanged.
    ``device_evaluate``: predictions are kept on the device (copied out of the engine's output buffer on its stream), the ground truth goes
    up without a blocking copy, one dvmvs.hip.ops.depth_errors launch per frame writes its eight metrics into a device table, the timer
    is the deferred one, and nothing waits for the device inside the loop; ONE download after it fetches everything (DeviceEvaluation).
    ``error_log`` (a list) then receives one float32 [8] row per prediction (``save_results(..., errors=error_log)``); it stays empty
    without ground truth or with ``evaluate=False``.  Default False: today's path, unchanged.
    ``fuse``: a ``dvmvs.tsdf.LiveFusion``: every prediction is also fused into its TSDF volume as it is made (``SceneResults``); after
    the run ``fuse.volume`` is the reconstruction.  "TRACKING LOST" lines do not touch it.  Default None: nothing changes."""
    frames = FrameInput(scene_folder, engine.device, device_preprocess)
    index = KeyframeIndex(keyframe_index_file, frames.scene.image_names, max_frames)
    results = SceneResults(frames, evaluate, device_evaluate, index.n_predictions, error_log, fuse)
    timer = InferenceTimer(deferred=device_evaluate)
    engine.new_sequence()
    for line, indices, upcoming in index:     # ``upcoming``: the index file says which keyframe is next (look-ahead)
        if frame_log is not None:
            frame_log.append(line)
        if indices is None:
            engine.reset()
            continue
        _run_frame(engine, frames, results, timer, indices, upcoming)
    return results.finish(timer)


def predict_online(engine: DepthEngine, scene_folder, evaluate=False, max_frames=None, frame_log=None, device_preprocess=False,
                   device_evaluate=False, error_log=None, fuse=None):
    """Feeds every frame of the scene to a KeyframeBuffer and predicts depth for the frames it accepts as keyframes.
    ``frame_log`` (a list) receives, in index-file syntax, what the buffer decided: one "ref meas1 ..." line per prediction and
    "TRACKING LOST" where it cleared itself -- the lines simulate_keyframe_index would write for the same poses.
    ``device_preprocess``, ``device_evaluate`` and ``error_log`` as in ``predict_offline``; the number of predictions is not known in
    advance here, so the device stack grows in blocks of 32 frames.  ``fuse`` as in ``predict_offline``."""
    frames = FrameInput(scene_folder, engine.device, device_preprocess)
    scene = frames.scene
    results = SceneResults(frames, evaluate, device_evaluate, 32, error_log, fuse)
    timer = InferenceTimer(deferred=device_evaluate)
    buffer = KeyframeBuffer(buffer_size=Config.test_keyframe_buffer_size, keyframe_pose_distance=Config.test_keyframe_pose_distance,
                            optimal_t_score=Config.test_optimal_t_measure, optimal_R_score=Config.test_optimal_R_measure,
                            store_return_indices=True)
    engine.new_sequence()
    n = len(scene.poses) if max_frames is None else min(max_frames, len(scene.poses))
    for i in range(n):
        response = buffer.try_new_keyframe(scene.poses[i], None, index=i)
        if response == 3:
            engine.reset()
            if frame_log is not None:
                frame_log.append("TRACKING LOST")
        if response != 1:
            continue
        indices = [i] + [frame[2] for frame in buffer.get_best_measurement_frames(Config.test_n_measurement_frames)]
        if frame_log is not None:
            frame_log.append(" ".join(scene.image_names[j] for j in indices))
        _run_frame(engine, frames, results, timer, indices)
    return results.finish(timer)


def predict_sharded(make_engine, scene_folders, keyframe_index_files, evaluate=True, max_frames=None, rank=None, world=None, fuse=None):
    """BASELINE.json configs[3]: independent scenes sharded over the ranks of one node (scene ``s`` belongs to rank
    ``s % world``, dvmvs.sharding), each run through ``predict_offline`` on this rank's engine; no data-path collective.
    ``make_engine()`` builds the rank's DepthEngine lazily (a rank that owns no scene builds none).  Returns
    ({scene number: (predictions, reference depths or None, InferenceTimer)}, (frames, seconds, frames/s) of the whole job).
    ``fuse``: a factory ``fuse(s)`` -> the ``dvmvs.tsdf.LiveFusion`` of scene number ``s`` (or None for that scene), called on the rank that
    owns the scene; the caller keeps the objects it hands out and reads their volumes after the job."""
    import time

    from dvmvs.sharding import reduce_throughput, run_sharded
    if len(scene_folders) != len(keyframe_index_files):
        raise ValueError("one keyframe index file per scene folder")
    state = {"engine": None}

    def run_scene(s):
        if state["engine"] is None:
            state["engine"] = make_engine()
        return predict_offline(state["engine"], scene_folders[s], keyframe_index_files[s], evaluate=evaluate, max_frames=max_frames,
                               fuse=fuse(s) if fuse is not None else None)

    t0 = time.perf_counter()
    results = run_sharded(len(scene_folders), run_scene, rank=rank, world=world)
    seconds = time.perf_counter() - t0
    frames = sum(len(r[0]) for r in results.values())
    # The reduction's device follows the BACKEND, not whether this rank built an engine: a rank that owns no scene (more ranks
    # than scenes) must still join an RCCL collective with a device tensor, or every other rank blocks in all_reduce.
    device = "cpu"
    if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_backend() == "nccl":
        device = torch.device("cuda", torch.cuda.current_device())
    return results, reduce_throughput(frames, seconds, device=device)

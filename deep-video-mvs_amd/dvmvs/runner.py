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
from dvmvs.dataset_loader import FrameUploader, PreprocessImage, load_depth_png, load_depth_png_u16, load_image, load_image_u8
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


def _to_device(image_hwc, device):
    return torch.from_numpy(np.ascontiguousarray(np.transpose(image_hwc, (2, 0, 1)))).float().unsqueeze(0).to(device)


def _preprocessor(scene, raw_image):
    return PreprocessImage(K=scene.K, old_width=raw_image.shape[1], old_height=raw_image.shape[0], new_width=Config.test_image_width,
                           new_height=Config.test_image_height, distortion_crop=Config.test_distortion_crop,
                           perform_crop=Config.test_perform_crop)


def _prepare(pre, raw, device, uploader):
    """Network input [1,3,h,w] on the device: on the host (numpy, then a blocking copy) or, with an ``uploader``, from the raw 8-bit frame
    in one kernel launch behind a pinned, non-blocking copy."""
    if uploader is None:
        return _to_device(pre.apply_rgb(raw, SCALE_RGB, MEAN_RGB, STD_RGB), device)
    return pre.apply_rgb_device(raw, SCALE_RGB, MEAN_RGB, STD_RGB, device=device, uploader=uploader)


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


def _run_frame(engine, scene, timer, device, reference_index, measurement_indices, evaluate, images=None, next_reference_index=None,
               prepared=None, next_measurement_indices=None, uploader=None, evaluation=None):
    """``next_reference_index``: the reference frame of the NEXT call when it is known (offline runs): its image is pre-processed now and
    handed to the engine as look-ahead (DepthEngine.step: its features are computed concurrently with this frame); ``prepared``
    (a dict) carries the pre-processed device image to that next call.  ``uploader`` (a FrameUploader; ``scene`` then loads raw 8- / 16-bit
    frames): images and the ground-truth depth are pre-processed on the device.  ``evaluation`` (a DeviceEvaluation): the prediction, the
    ground truth and their metrics stay on the device, nothing here waits for it, and (None, None) is returned."""
    raw = images[reference_index] if images is not None and reference_index in images else scene.image(reference_index)
    pre = _preprocessor(scene, raw)
    ref_image = prepared.pop(reference_index, None) if prepared is not None else None
    if ref_image is None:
        ref_image = _prepare(pre, raw, device, uploader)
    next_image = None
    if next_reference_index is not None and prepared is not None:
        raw_next = images[next_reference_index] if images is not None and next_reference_index in images else scene.image(next_reference_index)
        next_image = _prepare(_preprocessor(scene, raw_next), raw_next, device, uploader)
        prepared.clear()
        prepared[next_reference_index] = next_image
    ref_pose = torch.from_numpy(scene.poses[reference_index]).float().unsqueeze(0)   # poses / K stay on the host (engine.step)
    full_K = torch.from_numpy(pre.get_updated_intrinsics()).float().unsqueeze(0)
    meas_images, meas_poses = [], []
    for m in measurement_indices:
        if engine.cache_features and m in engine._feature_cache:
            meas_images.append(None)     # features of this keyframe are cached: no need to load / pre-process the image again
        else:
            raw_m = images[m] if images is not None and m in images else scene.image(m)
            meas_images.append(_prepare(pre, raw_m, device, uploader))
        meas_poses.append(torch.from_numpy(scene.poses[m]).float().unsqueeze(0))
    want_depth = bool(evaluate and scene.depth_names)
    depth_on_device = None
    slot = None
    if evaluation is not None:                   # the frame's slot; its ground truth is enqueued with the images, outside the timed region
        slot = evaluation.next_slot(pre.new_height, pre.new_width)
        if want_depth and uploader is not None:
            pre.apply_depth_device(scene.depth(reference_index), device=device, uploader=uploader, out=slot.gt.unsqueeze(0))
        elif want_depth:
            evaluation.stage(slot, pre.apply_depth(scene.depth(reference_index)))
    elif want_depth and uploader is not None:      # enqueued with the images, outside the timed region; fetched with the prediction
        depth_on_device = pre.apply_depth_device(scene.depth(reference_index), device=device, uploader=uploader)
    timer.record_start_time()
    ahead = {}
    if next_image is not None:
        ahead = dict(next_reference_image=next_image, next_frame_id=next_reference_index)
        if next_measurement_indices is not None:      # ... and its poses: the engine then also runs its sweep + encoder a frame ahead
            ahead.update(next_reference_pose=torch.from_numpy(scene.poses[next_reference_index]).float().unsqueeze(0),
                         next_measurement_poses=[torch.from_numpy(scene.poses[m]).float().unsqueeze(0) for m in next_measurement_indices],
                         next_measurement_ids=list(next_measurement_indices))
    depth = engine.step(ref_image, ref_pose, meas_images, meas_poses, full_K, frame_id=reference_index,
                        measurement_ids=list(measurement_indices), **ahead)
    timer.record_end_time_and_elapsed_time()
    if evaluation is not None:
        evaluation.commit(slot, depth)
        return None, None
    if depth_on_device is not None:              # one transfer for both maps (same size: the network's)
        both = torch.stack((depth.reshape(depth_on_device.shape[-2:]), depth_on_device[0])).cpu().numpy()
        return both[0], both[1]
    prediction = depth.cpu().numpy().squeeze()
    reference_depth = pre.apply_depth(scene.depth(reference_index)) if want_depth else None
    return prediction, reference_depth


def _finish_on_device(evaluation, timer, error_log):
    predictions, reference_depths = evaluation.finish(error_log)
    timer.resolve()
    return predictions, reference_depths, timer


def predict_offline(engine: DepthEngine, scene_folder, keyframe_index_file, evaluate=True, max_frames=None, frame_log=None,
                    device_preprocess=False, device_evaluate=False, error_log=None):
    """Runs the lines of a keyframe index file ("ref meas1 meas2 ..." or "TRACKING LOST") through ``engine``.
    ``frame_log`` (a list) receives the line each prediction belongs to: "ref meas1 ..." file names, or "TRACKING LOST".
    ``device_preprocess``: frames are loaded as 8-bit images, uploaded through a ring of pinned buffers and cropped / resized / normalised
    by one kernel launch each (dvmvs.hip.ops.preprocess_rgb; the ground-truth depth likewise, returned as float32) instead of by numpy
    on the host.  Default False: the host path, unchanged.
    ``device_evaluate``: predictions are kept on the device (copied out of the engine's output buffer on its stream), the ground truth goes
    up without a blocking copy, one dvmvs.hip.ops.depth_errors launch per frame writes its eight metrics into a device table, the timer
    is the deferred one, and nothing waits for the device inside the loop; ONE download after it fetches everything (DeviceEvaluation).
    ``error_log`` (a list) then receives one float32 [8] row per prediction (``save_results(..., errors=error_log)``); it stays empty
    without ground truth or with ``evaluate=False``.  Default False: today's path, unchanged."""
    scene = Scene(scene_folder, raw=device_preprocess)
    device = engine.device
    uploader = FrameUploader(device) if device_preprocess else None
    position = {name: i for i, name in enumerate(scene.image_names)}
    timer = InferenceTimer(deferred=device_evaluate)
    predictions, reference_depths = [], []
    engine.new_sequence()
    lines = [l.strip() for l in open(keyframe_index_file) if l.strip()][:max_frames]
    evaluation = None
    if device_evaluate:
        evaluation = DeviceEvaluation(device, evaluate and scene.depth_names, device_preprocess,
                                      capacity=sum(l != "TRACKING LOST" for l in lines))
    prepared = {}      # the next keyframe's pre-processed image (the index file says which frame that is: feature look-ahead)
    for n, line in enumerate(lines):
        if frame_log is not None:
            frame_log.append(line)
        if line == "TRACKING LOST":
            engine.reset()
            continue
        indices = [position[name] for name in line.split(" ")]
        upcoming = next((l for l in lines[n + 1:] if l != "TRACKING LOST"), None)
        next_indices = [position[name] for name in upcoming.split(" ")] if upcoming is not None else None
        prediction, reference_depth = _run_frame(engine, scene, timer, device, indices[0], indices[1:], evaluate,
                                                 next_reference_index=next_indices[0] if next_indices else None, prepared=prepared,
                                                 next_measurement_indices=next_indices[1:] if next_indices else None, uploader=uploader,
                                                 evaluation=evaluation)
        if evaluation is None:
            predictions.append(prediction)
            reference_depths.append(reference_depth)
    if evaluation is not None:
        return _finish_on_device(evaluation, timer, error_log)
    return predictions, (reference_depths if evaluate and scene.depth_names else None), timer


def predict_online(engine: DepthEngine, scene_folder, evaluate=False, max_frames=None, frame_log=None, device_preprocess=False,
                   device_evaluate=False, error_log=None):
    """Feeds every frame of the scene to a KeyframeBuffer and predicts depth for the frames it accepts as keyframes.
    ``frame_log`` (a list) receives, in index-file syntax, what the buffer decided: one "ref meas1 ..." line per prediction and
    "TRACKING LOST" where it cleared itself -- the lines simulate_keyframe_index would write for the same poses.
    ``device_preprocess``, ``device_evaluate`` and ``error_log`` as in ``predict_offline``; the number of predictions is not known in
    advance here, so the device stack grows in blocks of 32 frames."""
    scene = Scene(scene_folder, raw=device_preprocess)
    device = engine.device
    uploader = FrameUploader(device) if device_preprocess else None
    evaluation = DeviceEvaluation(device, evaluate and scene.depth_names, device_preprocess, capacity=32) if device_evaluate else None
    buffer = KeyframeBuffer(buffer_size=Config.test_keyframe_buffer_size, keyframe_pose_distance=Config.test_keyframe_pose_distance,
                            optimal_t_score=Config.test_optimal_t_measure, optimal_R_score=Config.test_optimal_R_measure,
                            store_return_indices=True)
    timer = InferenceTimer(deferred=device_evaluate)
    predictions, reference_depths = [], []
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
        measurement_indices = [frame[2] for frame in buffer.get_best_measurement_frames(Config.test_n_measurement_frames)]
        if frame_log is not None:
            frame_log.append(" ".join(scene.image_names[j] for j in [i] + measurement_indices))
        prediction, reference_depth = _run_frame(engine, scene, timer, device, i, measurement_indices, evaluate, uploader=uploader,
                                                 evaluation=evaluation)
        if evaluation is None:
            predictions.append(prediction)
            reference_depths.append(reference_depth)
    if evaluation is not None:
        return _finish_on_device(evaluation, timer, error_log)
    return predictions, (reference_depths if evaluate and scene.depth_names else None), timer


def predict_sharded(make_engine, scene_folders, keyframe_index_files, evaluate=True, max_frames=None, rank=None, world=None):
    """BASELINE.json configs[3]: independent scenes sharded over the ranks of one node (scene ``s`` belongs to rank
    ``s % world``, dvmvs.sharding), each run through ``predict_offline`` on this rank's engine; no data-path collective.
    ``make_engine()`` builds the rank's DepthEngine lazily (a rank that owns no scene builds none).  Returns
    ({scene number: (predictions, reference depths or None, InferenceTimer)}, (frames, seconds, frames/s) of the whole job)."""
    import time

    from dvmvs.sharding import reduce_throughput, run_sharded
    if len(scene_folders) != len(keyframe_index_files):
        raise ValueError("one keyframe index file per scene folder")
    state = {"engine": None}

    def run_scene(s):
        if state["engine"] is None:
            state["engine"] = make_engine()
        return predict_offline(state["engine"], scene_folders[s], keyframe_index_files[s], evaluate=evaluate, max_frames=max_frames)

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

"""Scene runners of the MVDepthNet, GP-MVS and DPSNet baselines: the loops of the reference's dvmvs/baselines/mvdepthnet/run-testing.py,
dvmvs/baselines/gpmvs/run-testing.py and dvmvs/baselines/dpsnet/run-testing.py on the MI355X, without cv2 / path / tqdm / scipy.

Per frame, one dvmvs::rgb_sweep launch writes the encoder's 67-channel input (the normalised reference image and its 64-plane SAD cost
volume, 0.5 - 50 m) into a buffer the runner keeps; the encoder and decoder run on MIOpen; the prediction is 1 / clamp(disp1, 0.02, 2).
GP-MVS filters the encoder's conv5 between frames with dvmvs::gp_filter_step: the 2x2 algebra of the filter depends on the poses only
and is evaluated on the host (GPFilter), the float64 state stays on the device, and a frame has no host synchronisation between the
sweep and the prediction.

Reference behaviour that is kept: preprocessing with scale 1, mean 81, std 35 at the full 320x256 (no crop, K from
get_updated_intrinsics()); "TRACKING LOST" lines are skipped and do not reset the GP state; on a scene's first frame GP-MVS measures the
pose distance to the LAST measurement frame of that line; the timed region runs from the cost volume to the inverted prediction.

DPSNet (predict_dpsnet) differs: 320x240, scale 255 with mean and std 0.5, PSNet(64, 0.5); the network gets the relative poses
(inv(measurement) @ reference)[0:3], taken in float64 on the host, K and np.linalg.inv(K); the timed region is the network call and its
second output is the prediction.
"""
import glob
import os

import numpy as np
import torch

from dvmvs.baselines.networks import Decoder, Encoder
from dvmvs.baselines.dpsnet.dpsnet import PSNet
from dvmvs.baselines.gpmvs.gplayer import GPlayer
from dvmvs.hip import ops
from dvmvs.pose_algebra import sweep_matrices_host
from dvmvs.runner import FrameInput, KeyframeIndex, SceneResults
from dvmvs.utils import InferenceTimer, pose_distance

WIDTH, HEIGHT = 320, 256
MIN_DEPTH, MAX_DEPTH, N_DEPTH_LEVELS = 0.5, 50.0, 64
SCALE_RGB = 1.0
MEAN_RGB = [81.0, 81.0, 81.0]
STD_RGB = [35.0, 35.0, 35.0]
LATENT = (512, 8, 10)        # conv5 of a 256x320 frame
DPS_WIDTH, DPS_HEIGHT = 320, 240
DPS_NLABEL, DPS_MIN_DEPTH = 64, 0.5
DPS_SCALE_RGB = 255.0
DPS_MEAN_RGB = [0.5, 0.5, 0.5]
DPS_STD_RGB = [0.5, 0.5, 0.5]


# ----------------------------------------------------------------------------------------------------------------------
# checkpoints
# ----------------------------------------------------------------------------------------------------------------------
def load_checkpoint(module, checkpoint):
    """Loads a published checkpoint into ``module``: a plain state dict, a ``module.``-prefixed one (saved through DataParallel), or a
    combined file ``{'state_dict': ...}`` holding several modules' parameters, of which the keys of ``module`` are taken
    (mvdepthnet/run-testing.py:35-42)."""
    if isinstance(checkpoint, (str, os.PathLike)):
        checkpoint = torch.load(checkpoint, map_location="cpu", weights_only=True)
    combined = "state_dict" in checkpoint and isinstance(checkpoint["state_dict"], dict)
    state = checkpoint["state_dict"] if combined else checkpoint
    state = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state.items()}
    if combined:
        own = module.state_dict()
        own.update({k: v for k, v in state.items() if k in own})
        state = own
    module.load_state_dict(state)
    return module


def _only(folder, pattern):
    files = sorted(glob.glob(os.path.join(str(folder), pattern)))
    if not files:
        raise FileNotFoundError(f"no checkpoint matching {pattern!r} in {folder}")
    return files[0]


def build_mvdepthnet(weights_folder=None, device="cuda", seed=0):
    """(encoder, decoder) in eval mode on ``device``.  ``weights_folder``: files ``*encoder*`` and ``*decoder*`` (the fine-tuned
    weights), or ``pretrained_mvdepthnet_combined`` (the original combined file); None = seeded weights (tests, benchmarks)."""
    torch.manual_seed(seed)
    encoder, decoder = Encoder(), Decoder()
    if weights_folder is not None:
        combined = os.path.join(str(weights_folder), "pretrained_mvdepthnet_combined")
        if os.path.exists(combined):
            checkpoint = torch.load(combined, map_location="cpu", weights_only=True)
            load_checkpoint(encoder, checkpoint)
            load_checkpoint(decoder, checkpoint)
        else:
            load_checkpoint(encoder, _only(weights_folder, "*encoder*"))
            load_checkpoint(decoder, _only(weights_folder, "*decoder*"))
    return encoder.to(device).eval(), decoder.to(device).eval()


def build_gpmvs(weights_folder=None, device="cuda", seed=0):
    """(encoder, decoder, gplayer) in eval mode on ``device`` from files ``*encoder*``, ``*decoder*``, ``*gplayer*`` (plain,
    ``module.``-prefixed or ``{'state_dict': ...}``); None = seeded weights."""
    torch.manual_seed(seed)
    encoder, decoder, gplayer = Encoder(), Decoder(), GPlayer(device="cpu")
    if weights_folder is not None:
        load_checkpoint(encoder, _only(weights_folder, "*encoder*"))
        load_checkpoint(decoder, _only(weights_folder, "*decoder*"))
        load_checkpoint(gplayer, _only(weights_folder, "*gplayer*"))
    gplayer.device = torch.device(device)
    return encoder.to(device).eval(), decoder.to(device).eval(), gplayer.to(device).eval()


def build_dpsnet(weights_folder=None, device="cuda", seed=0):
    """PSNet(64, 0.5) in eval mode on ``device`` from a file ``*dpsnet*`` (a plain state dict: the fine-tuned weights, or
    ``{'state_dict': ...}``: the original ones); None = seeded weights."""
    torch.manual_seed(seed)
    dpsnet = PSNet(DPS_NLABEL, DPS_MIN_DEPTH)
    if weights_folder is not None:
        load_checkpoint(dpsnet, _only(weights_folder, "*dpsnet*"))
    return dpsnet.to(device).eval()


# ----------------------------------------------------------------------------------------------------------------------
# GP-MVS filter: host algebra of the poses, device state
# ----------------------------------------------------------------------------------------------------------------------
def gp_transition(lam, dt):
    """expm(F dt) for F = [[0, 1], [-lam^2, -2 lam]] (double eigenvalue -lam), in closed form: e^{-lam dt} [[1 + lam dt, dt],
    [-lam^2 dt, 1 - lam dt]]."""
    e = np.exp(-lam * dt)
    return e * np.array([[1.0 + lam * dt, dt], [-lam * lam * dt, 1.0 - lam * dt]])


class GPFilter:
    """The 2x2 part of GP-MVS's Kalman filter (gpmvs/run-testing.py:97-106, 179-190) in float64 on the host: per frame, the transition
    A and gain k that dvmvs::gp_filter_step applies to the [2, N] state mean on the device."""

    def __init__(self, gamma2_log, ell_log, sigma2_log):
        self.gamma2, ell, self.sigma2 = np.exp(gamma2_log), np.exp(ell_log), np.exp(sigma2_log)
        self.lam = np.sqrt(3) / ell
        self.Pinf = np.array([[self.gamma2, 0.0], [0.0, self.gamma2 * self.lam ** 2]])
        self.reset()

    @classmethod
    def from_gplayer(cls, gplayer):
        return cls(*(p.detach().double().cpu().reshape(-1)[0].item() for p in (gplayer.gamma2, gplayer.ell, gplayer.sigma2)))

    def reset(self):
        """A new scene: P = Pinf; the next step starts the state mean from zero."""
        self.P = self.Pinf.copy()
        self.fresh = True

    def step(self, dt):
        """Advances the covariance by one frame ``dt`` apart; returns (A row-major [4], k [2], reset) for gp_filter_step."""
        A = gp_transition(self.lam, dt)
        Q = self.Pinf - A.dot(self.Pinf).dot(A.T)
        P = A.dot(self.P).dot(A.T) + Q
        s = P[0, 0] + self.sigma2
        k = P[:, 0] / s
        self.P = P - np.outer(k, P[0, :])
        reset, self.fresh = self.fresh, False
        return [float(v) for v in A.reshape(-1)], [float(k[0]), float(k[1])], reset


# ----------------------------------------------------------------------------------------------------------------------
# one frame
# ----------------------------------------------------------------------------------------------------------------------
class BaselineFrame:
    """One frame of either baseline on preprocessed device images and host poses.  Keeps the 67-channel encoder input buffer and,
    for GP-MVS, the float64 filter state on the device."""

    def __init__(self, encoder, decoder, device, gp=None):
        self.encoder, self.decoder, self.gp = encoder, decoder, gp
        self.device = torch.device(device)
        self.fused = None
        self.state = torch.zeros((2, int(np.prod(LATENT))), dtype=torch.float64, device=self.device) if gp is not None else None

    def sweep(self, reference_image, measurement_images, reference_pose, measurement_poses, K):
        """[B, 67, H, W]: image in channels 0..2, the SAD cost volume of ``measurement_images`` in 3..66 (one launch).  Poses [B,4,4]
        and K [B,3,3] are float32 host tensors; their sweep matrices are evaluated with the reference's fp32 expressions."""
        B, C, H, W = reference_image.shape
        if self.fused is None or self.fused.shape != (B, 3 + N_DEPTH_LEVELS, H, W):
            self.fused = torch.empty((B, 3 + N_DEPTH_LEVELS, H, W), dtype=torch.float32, device=self.device)
        Hm, kt = sweep_matrices_host(reference_pose, list(measurement_poses), K)
        Hm = Hm.pin_memory().to(self.device, non_blocking=True)
        kt = kt.pin_memory().to(self.device, non_blocking=True)
        ops.rgb_sweep(self.fused, reference_image, list(measurement_images), Hm, kt, MIN_DEPTH, MAX_DEPTH, N_DEPTH_LEVELS, 3, True)
        return self.fused

    def __call__(self, reference_image, measurement_images, reference_pose, measurement_poses, K, dt=None, outputs=None):
        """Depth [B,1,H,W].  GP-MVS needs ``dt``, the pose distance to the previous frame.  ``outputs`` (a dict) receives conv5 and,
        for GP-MVS, Z."""
        fused = self.sweep(reference_image, measurement_images, reference_pose, measurement_poses, K)
        conv5, conv4, conv3, conv2, conv1 = self.encoder.forward_fused(fused)
        if self.gp is not None:
            A, k, reset = self.gp.step(dt)
            latent = ops.gp_filter_step(self.state, conv5.reshape(-1), A, k, reset).view_as(conv5)
        else:
            latent = conv5
        if outputs is not None:
            outputs["conv5"] = conv5
            outputs["Z"] = latent
        disp = self.decoder(latent, conv4, conv3, conv2, conv1)[0]
        return 1.0 / torch.clamp(disp, min=0.02, max=2.0)


# ----------------------------------------------------------------------------------------------------------------------
# scene loops
# ----------------------------------------------------------------------------------------------------------------------
def _index_file_fields(keyframe_index_file):
    """(keyframing type, dataset name, scene name, number of measurement frames) from "keyframe+dataset+scene+nmeas+N"."""
    keyframing_type, dataset_name, scene_name, _, n_measurement_frames = os.path.basename(str(keyframe_index_file)).split("+")
    return keyframing_type, dataset_name, scene_name, n_measurement_frames


def system_name(method, keyframe_index_file, finetuned=True, size=(WIDTH, HEIGHT)):
    """Result name of the run-testing scripts; ``size`` = (width, height) of the network input (DPSNet: 320 x 240)."""
    keyframing_type, dataset_name, _, n_measurement_frames = _index_file_fields(keyframe_index_file)
    return "{}_{}_{}_{}_{}_{}_{}".format(keyframing_type, dataset_name, size[0], size[1], n_measurement_frames, method,
                                         "finetuned" if finetuned else "without_ft")


def _predict(method_inputs, device, size, rgb, scene_folder, keyframe_index_file, evaluate, max_frames, device_preprocess, device_evaluate,
             error_log, fuse=None):
    """The loop of the three baselines: "TRACKING LOST" lines are skipped.  ``method_inputs(scene, pre, reference_index,
    measurement_indices)`` evaluates what the method's network takes besides the images (poses, intrinsics), outside the timed region,
    and returns the timed call ``(reference_image, measurement_images) -> depth``."""
    frames = FrameInput(scene_folder, device, device_preprocess, rgb=rgb, size=size, crop=(0, False))
    index = KeyframeIndex(keyframe_index_file, frames.scene.image_names, max_frames)
    results = SceneResults(frames, evaluate, device_evaluate, index.n_predictions, error_log, fuse)
    timer = InferenceTimer(deferred=device_evaluate)
    with torch.no_grad():
        for _, indices, _ in index:
            if indices is None:
                continue
            reference_index, measurement_indices = indices[0], indices[1:]
            raw = frames.scene.image(reference_index)
            pre = frames.preprocessor(raw)
            reference_image = frames.prepare(pre, raw)
            measurement_images = [frames.image(pre, m) for m in measurement_indices]
            network = method_inputs(frames.scene, pre, reference_index, measurement_indices)
            results.begin(pre, reference_index, raw=raw)
            timer.record_start_time()
            depth = network(reference_image, measurement_images)
            timer.record_end_time_and_elapsed_time()
            results.add(depth)
    return results.finish(timer)


def _predict_baseline(frame, scene_folder, keyframe_index_file, evaluate, max_frames, device_preprocess=False, device_evaluate=False,
                      error_log=None, fuse=None):
    """MVDepthNet and GP-MVS (``frame``: a BaselineFrame): float32 host poses and K; GP-MVS also gets ``dt``, the pose distance to the
    previous prediction's frame, which a tracking loss does not reset."""
    previous_index = None
    if frame.gp is not None:
        frame.gp.reset()

    def inputs(scene, pre, reference_index, measurement_indices):
        nonlocal previous_index
        reference_pose, measurement_poses = scene.pose(reference_index), [scene.pose(m) for m in measurement_indices]
        K = FrameInput.intrinsics(pre)
        dt = None
        if frame.gp is not None:
            if previous_index is None:
                previous_index = measurement_indices[-1]     # the reference's leaked loop variable
            dt = pose_distance(scene.poses[reference_index], scene.poses[previous_index])[0]
        previous_index = reference_index
        return lambda reference_image, measurement_images: frame(reference_image, measurement_images, reference_pose, measurement_poses, K,
                                                                 dt=dt)

    return _predict(inputs, frame.device, (WIDTH, HEIGHT), (SCALE_RGB, MEAN_RGB, STD_RGB), scene_folder, keyframe_index_file, evaluate,
                    max_frames, device_preprocess, device_evaluate, error_log, fuse)


def predict_mvdepthnet(scene_folder, keyframe_index_file, weights_folder=None, evaluate=True, max_frames=None, device="cuda",
                       device_preprocess=False, device_evaluate=False, error_log=None, fuse=None):
    """MVDepthNet over the lines of a keyframe index file.  Returns (predictions, reference depths or None, InferenceTimer).
    ``device_preprocess``: raw 8-bit frames are uploaded through a pinned ring and pre-processed by dvmvs.hip.ops.preprocess_rgb (the
    ground-truth depth by preprocess_depth, float32) instead of by numpy on the host.
    ``device_evaluate``: predictions, ground truth and their eight error metrics (one dvmvs.hip.ops.depth_errors launch per frame) stay on
    the device until the scene is done, the timer is the deferred one, and one download fetches everything; ``error_log`` (a list)
    receives a float32 [8] row per prediction for ``save_results(..., errors=error_log)`` (dvmvs.runner.predict_offline).
    ``fuse``: a ``dvmvs.tsdf.LiveFusion`` that also receives every prediction as it is made (dvmvs.runner.predict_offline)."""
    encoder, decoder = build_mvdepthnet(weights_folder, device)
    return _predict_baseline(BaselineFrame(encoder, decoder, device), scene_folder, keyframe_index_file, evaluate, max_frames,
                             device_preprocess, device_evaluate, error_log, fuse)


def predict_gpmvs(scene_folder, keyframe_index_file, weights_folder=None, evaluate=True, max_frames=None, device="cuda",
                  device_preprocess=False, device_evaluate=False, error_log=None, fuse=None):
    """GP-MVS over the lines of a keyframe index file.  Returns (predictions, reference depths or None, InferenceTimer).
    ``device_preprocess``, ``device_evaluate``, ``error_log`` and ``fuse`` as in ``predict_mvdepthnet``."""
    encoder, decoder, gplayer = build_gpmvs(weights_folder, device)
    frame = BaselineFrame(encoder, decoder, device, gp=GPFilter.from_gplayer(gplayer))
    return _predict_baseline(frame, scene_folder, keyframe_index_file, evaluate, max_frames, device_preprocess, device_evaluate, error_log,
                             fuse)


def dpsnet_relative_pose(reference_pose, measurement_pose):
    """[1,3,4] float32: (inv(measurement) @ reference)[0:3] in float64 on the host, then cast (dpsnet/run-testing.py:110-112)."""
    return torch.from_numpy((np.linalg.inv(measurement_pose) @ reference_pose)[0:3, :]).float().unsqueeze(0)


def predict_dpsnet(scene_folder, keyframe_index_file, weights_folder=None, evaluate=True, max_frames=None, device="cuda",
                   device_preprocess=False, device_evaluate=False, error_log=None, fuse=None):
    """DPSNet over the lines of a keyframe index file.  Returns (predictions, reference depths or None, InferenceTimer).
    ``device_preprocess``, ``device_evaluate``, ``error_log`` and ``fuse`` as in ``predict_mvdepthnet``."""
    dpsnet = build_dpsnet(weights_folder, device)

    def inputs(scene, pre, reference_index, measurement_indices):
        poses = [dpsnet_relative_pose(scene.poses[reference_index], scene.poses[m]).to(device) for m in measurement_indices]
        camera_k = pre.get_updated_intrinsics()
        K = torch.from_numpy(camera_k).float().unsqueeze(0).to(device)
        K_inv = torch.from_numpy(np.linalg.inv(camera_k)).float().unsqueeze(0).to(device)
        return lambda reference_image, measurement_images: dpsnet(reference_image, measurement_images, poses, K, K_inv)[1]

    return _predict(inputs, device, (DPS_WIDTH, DPS_HEIGHT), (DPS_SCALE_RGB, DPS_MEAN_RGB, DPS_STD_RGB), scene_folder, keyframe_index_file,
                    evaluate, max_frames, device_preprocess, device_evaluate, error_log, fuse)


def live_fusion_for_scene(scene_folder, size, voxel_size, max_depth, batch, device="cuda"):
    """The ``LiveFusion`` of ``--fuse``: its volume spans the frusta of ALL the scene's poses cut at ``max_depth`` (``frustum_bounds``, with
    the reconstruction program's 5 % margin), at the intrinsics of a ``size`` = (width, height) prediction -- sized before any depth exists."""
    from dvmvs.runner import Scene, _preprocessor
    from dvmvs.tsdf import LiveFusion, TSDFFusion
    scene = Scene(scene_folder)
    K = _preprocessor(scene, scene.image(0), size, (0, False)).get_updated_intrinsics()
    bounds = TSDFFusion.frustum_bounds(list(scene.poses), K, size[1], size[0], max_depth) * 1.05
    return LiveFusion(bounds, voxel_size=voxel_size, max_depth=max_depth, batch=batch, device=device)


def sparse_live_fusion(voxel_size, max_depth, batch, max_bricks, device="cuda"):
    """The ``LiveFusion`` of ``--fuse --fuse_sparse``: no bounds, so nothing of the scene is read -- not its poses, not its intrinsics; the
    frames go into a ``SparseTSDFVolume`` of ``max_bricks`` bricks that allocates what they touch."""
    from dvmvs.tsdf import LiveFusion
    return LiveFusion(None, voxel_size=voxel_size, max_depth=max_depth, batch=batch, device=device, max_bricks=max_bricks)


def fusion_for_arguments(args, size):
    """The ``LiveFusion`` that the parsed ``--fuse*`` flags ask for, or None: with ``--fuse_sparse`` without a look at the scene."""
    if not args.fuse:
        if args.fuse_sparse:
            raise SystemExit("--fuse_sparse says how --fuse fuses: it needs --fuse")
        return None
    if args.fuse_sparse:
        return sparse_live_fusion(args.fuse_voxel_size, args.fuse_max_depth, args.fuse_batch, args.fuse_bricks)
    return live_fusion_for_scene(args.scene_folder, size, args.fuse_voxel_size, args.fuse_max_depth, args.fuse_batch)


def build_parser(method):
    """The parser of ``python -m dvmvs.baselines.<method>``."""
    import argparse
    parser = argparse.ArgumentParser(prog=f"python -m dvmvs.baselines.{method}")
    parser.add_argument("scene_folder")
    parser.add_argument("keyframe_index_file")
    parser.add_argument("--weights", default=None, help="checkpoint folder (default: seeded weights)")
    parser.add_argument("--without-ft", action="store_true", help="name the results '..._without_ft' (original weights)")
    parser.add_argument("--out", default=".", help="folder for the .npz results")
    parser.add_argument("--max-frames", type=int, default=None)
    parser.add_argument("--device-preprocess", action="store_true",
                        help="crop / resize / normalise the raw 8-bit frames on the GPU (one launch per image) instead of with numpy")
    parser.add_argument("--device-evaluate", action="store_true",
                        help="keep predictions and ground truth on the GPU and evaluate the error metrics there (one launch per frame, one "
                             "download per scene) instead of fetching every frame and evaluating with numpy")
    parser.add_argument("--fuse", action="store_true",
                        help="fuse every prediction into a TSDF volume while the scene runs and write <out>/<system>_<scene>_live_complete.ply")
    parser.add_argument("--fuse_voxel_size", default=0.025, type=float)
    parser.add_argument("--fuse_max_depth", default=5.0, type=float)
    parser.add_argument("--fuse_batch", default=8, type=int, help="frames fused per launch")
    parser.add_argument("--fuse_sparse", action="store_true",
                        help="with --fuse: fuse into a brick-hashed volume that needs no bounds, so the scene's poses are not read in advance")
    parser.add_argument("--fuse_bricks", default=65536, type=int, help="with --fuse_sparse: the pool's capacity in bricks of 8 x 8 x 8 voxels")
    return parser


def main(method, argv=None):
    """``python -m dvmvs.baselines.{mvdepthnet,gpmvs,dpsnet} SCENE_FOLDER INDEX_FILE [--weights DIR] [--without-ft] [--out DIR]
    [--device-preprocess] [--device-evaluate] [--fuse [--fuse_voxel_size M] [--fuse_max_depth M] [--fuse_batch N]
    [--fuse_sparse [--fuse_bricks N]]]``."""
    from dvmvs.utils import save_results
    args = build_parser(method).parse_args(argv)
    predict = {"mvdepthnet": predict_mvdepthnet, "gpmvs": predict_gpmvs, "dpsnet": predict_dpsnet}[method]
    size = (DPS_WIDTH, DPS_HEIGHT) if method == "dpsnet" else (WIDTH, HEIGHT)
    error_log = []
    fuse = fusion_for_arguments(args, size)
    predictions, reference_depths, timer = predict(args.scene_folder, args.keyframe_index_file, args.weights, max_frames=args.max_frames,
                                                  device_preprocess=args.device_preprocess, device_evaluate=args.device_evaluate,
                                                  error_log=error_log, fuse=fuse)
    timer.print_statistics()
    name, scene_name = system_name(method, args.keyframe_index_file, finetuned=not args.without_ft, size=size), \
        _index_file_fields(args.keyframe_index_file)[2]
    save_results(predictions=predictions, groundtruths=reference_depths, errors=error_log if args.device_evaluate else None,
                 system_name=name, scene_name=scene_name, save_folder=args.out)
    if fuse is not None:
        from dvmvs.tsdf import TSDFFusion
        os.makedirs(args.out, exist_ok=True)
        mesh = os.path.join(args.out, f"{name}_{scene_name}_live")
        print("Saving mesh to", mesh)
        TSDFFusion.meshwrite(mesh + "_complete.ply", *fuse.volume.get_mesh())

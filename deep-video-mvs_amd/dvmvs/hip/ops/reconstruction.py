"""The ops around a reconstruction (inference only): frame pre-processing, depth errors, ray-casting and batched fusion of a TSDF volume,
nearest-point distances with the 3-D metrics they reduce to and the point sets they are taken between, and the multi-view consistency
filter."""
from typing import Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from dvmvs.hip import _capi
from dvmvs.hip.ops import _workspace
from dvmvs.hip.ops._common import EUNSUPPORTED, check_tensors, launch, opt_ptr, out_or_new, ptr


# ----------------------------------------------------------------------------------------------------------------------
# frame pre-processing: raw 8-bit frames / 16-bit depth maps -> network input, one launch for N frames
# ----------------------------------------------------------------------------------------------------------------------
def _raw_frames(name, raw, dtypes, channels):
    """``raw`` as [N,H,W(,3)] on the device with unit element stride inside a row and frames H rows apart; returns (tensor, N, H, W)."""
    check_tensors(name, raw, dtype=dtypes)
    want = 3 if channels else 2
    if raw.dim() == want:
        raw = raw.unsqueeze(0)
    if raw.dim() != want + 1 or (channels and raw.shape[-1] != 3) or raw.numel() == 0:
        layout = "[N,H,W,3] or [H,W,3]" if channels else "[N,H,W] or [H,W]"
        raise ValueError(f"dvmvs::{name}: expected non-empty frames {layout}, got {tuple(raw.shape)}")
    N, H, W = raw.shape[:3]
    return raw, N, H, W


def _check_crop(name, H, W, crop_x, crop_y, new_height, new_width):
    if new_height < 1 or new_width < 1 or crop_x < 0 or crop_y < 0 or W - 2 * crop_x < 1 or H - 2 * crop_y < 1:
        raise ValueError(f"dvmvs::{name}: crop ({crop_x}, {crop_y}) of a {H}x{W} frame to {new_height}x{new_width} leaves no pixels")


def preprocess_rgb(raw: Tensor, crop_x: int, crop_y: int, new_height: int, new_width: int, scale: float, mean: Sequence[float],
                   std: Sequence[float], normalize: bool = True, out: Optional[Tensor] = None) -> Tensor:
    """``PreprocessImage.apply_rgb`` on the device, one launch: ``raw`` uint8 [N,H,W,3] (or [H,W,3]) interleaved RGB on the GPU -> float32
    [N,3,new_height,new_width]: ``crop_x`` columns / ``crop_y`` rows dropped on each side, bilinear resampling (half-pixel centres, clamped
    edges), ``(v / scale - mean[c]) / std[c]`` unless ``normalize`` is False (then the resampled 0..255 values), HWC -> CHW.  Rows may be
    padded (``raw.stride(1) >= 3 W`` bytes; pixels and channels dense, frames H rows apart).  ``out``: a float32 [N,3,new_height,new_width]
    view whose three planes are dense and whose batch stride is free (a slot of a larger buffer); it is returned.  Tap indices and blend
    weights are the host function's bit for bit (evaluated in double); the fp32 blends follow its order without FMA contraction.  Runs on
    the current stream."""
    raw, N, H, W = _raw_frames("preprocess_rgb", raw, torch.uint8, True)
    crop_x, crop_y, new_height, new_width = int(crop_x), int(crop_y), int(new_height), int(new_width)
    _check_crop("preprocess_rgb", H, W, crop_x, crop_y, new_height, new_width)
    if raw.stride(3) != 1 or raw.stride(2) != 3 or raw.stride(1) < 3 * W or (N > 1 and raw.stride(0) != H * raw.stride(1)):
        raw = raw.contiguous()
    normalize = bool(normalize)
    if normalize:
        if len(mean) != 3 or len(std) != 3:
            raise ValueError("dvmvs::preprocess_rgb: mean and std have 3 entries")
        if float(scale) == 0.0 or any(float(v) == 0.0 for v in std):
            raise ValueError("dvmvs::preprocess_rgb: scale and std must be non-zero")
    frame = 3 * new_height * new_width
    if out is None:
        out = torch.empty((N, 3, new_height, new_width), dtype=torch.float32, device=raw.device)
    else:     # not ``out_or_new``: the planes must be dense, the batch stride is free
        check_tensors("preprocess_rgb", out)
        check_tensors("preprocess_rgb", out, label="out", shape=(N, 3, new_height, new_width), device=raw.device)
        if tuple(out.stride()[1:]) != (new_height * new_width, new_width, 1) or (N > 1 and out.stride(0) < frame):
            raise ValueError(f"dvmvs::preprocess_rgb: out must have dense planes, got strides {tuple(out.stride())}")
    launch("dvmvs_preprocess_rgb_fwd", raw.device, ptr(raw), ptr(out), N, H, W, raw.stride(1), crop_x, crop_y, new_height, new_width,
           out.stride(0) if N > 1 else frame, float(scale) if normalize else 1.0, _capi.float_array(mean) if normalize else None,
           _capi.float_array(std) if normalize else None, int(normalize))
    return out


# 16-bit unsigned frames on the device: torch.uint16 where this torch build has it; an int16 tensor is read as its bit pattern
_U16_DTYPES = tuple(d for d in (getattr(torch, "uint16", None), torch.int16) if d is not None)


def preprocess_depth(raw: Tensor, crop_x: int, crop_y: int, new_height: int, new_width: int, scaling: float = 1000.0,
                     out: Optional[Tensor] = None) -> Tensor:
    """``PreprocessImage.apply_depth(load_depth_png(...))`` on the device, one launch: ``raw`` 16-bit unsigned depth maps [N,H,W] (or [H,W])
    in millimetres on the GPU -> float32 [N,new_height,new_width] in metres: crop, nearest resampling (source index
    ``min(int(x * (w / new_w)), w - 1)``), ``float32(d / scaling)`` with the division in double.  ``raw`` is a ``torch.uint16`` tensor (this
    torch build has the dtype and can hold and copy it on the device) or, equivalently, an ``int16`` tensor whose bits are read as unsigned
    (``uint16_array.view(np.int16)``).  ``out``: a contiguous float32 [N,new_height,new_width] tensor; it is returned."""
    raw, N, H, W = _raw_frames("preprocess_depth", raw, _U16_DTYPES, False)
    crop_x, crop_y, new_height, new_width = int(crop_x), int(crop_y), int(new_height), int(new_width)
    _check_crop("preprocess_depth", H, W, crop_x, crop_y, new_height, new_width)
    if float(scaling) == 0.0:
        raise ValueError("dvmvs::preprocess_depth: scaling must be non-zero")
    raw = raw.contiguous()
    if out is not None:
        check_tensors("preprocess_depth", out)
    out = out_or_new("preprocess_depth", out, (N, new_height, new_width), torch.float32, raw.device)
    launch("dvmvs_preprocess_depth_fwd", raw.device, ptr(raw), ptr(out), N, H, W, crop_x, crop_y, new_height, new_width, float(scaling))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# depth evaluation: the eight metrics of dvmvs.errors.compute_errors for N frames, one launch
# ----------------------------------------------------------------------------------------------------------------------
def depth_errors_workspace(device, n_frames, pixels):
    """Persistent workspace of ``depth_errors`` for (device, N, pixels): zero-filled once here; every call leaves its ticket words zero
    (contract in include/dvmvs_hip.h).  As with ``sweep_workspace``, calls that share it must be ordered with respect to each other (one
    stream per process); allocated outside any graph capture when the first (eager / warm-up) call of a size happens."""
    nbytes = _capi.lib().dvmvs_depth_errors_workspace_bytes(n_frames, pixels)
    if nbytes == 0:
        _capi.check(EUNSUPPORTED, "dvmvs_depth_errors_workspace_bytes")
    return _workspace.zeroed("depth_errors", device, (n_frames, pixels), nbytes, torch.float64)


def _frames_2d(name, t):
    """[H,W], [N,H,W] or [N,1,H,W] -> (N, pixels)."""
    if t.dim() == 2:
        return 1, t.shape[0] * t.shape[1]
    if t.dim() == 3:
        return t.shape[0], t.shape[1] * t.shape[2]
    if t.dim() == 4 and t.shape[1] == 1:
        return t.shape[0], t.shape[2] * t.shape[3]
    raise ValueError(f"dvmvs::{name}: expected depth maps [H,W], [N,H,W] or [N,1,H,W], got {tuple(t.shape)}")


def depth_errors(gt: Tensor, pred: Tensor, max_depth: float = float("inf"), out: Optional[Tensor] = None,
                 counts: Optional[Tensor] = None) -> Tensor:
    """``dvmvs.errors.compute_errors`` on the device, one launch for all frames: ``gt`` and ``pred`` float32 depth maps [H,W], [N,H,W] or
    [N,1,H,W] on the GPU -> float32 [N,8] (abs_error, abs_relative_error, abs_inverse_error, squared_relative_error, rmse, ratio_125,
    ratio_125_2, ratio_125_3) over the pixels with ``0.5 <= gt <= max_depth``; a frame without such a pixel gives eight NaNs.  The
    per-pixel terms are the host function's fp32 operations; they are summed in float64 in a fixed order, so a row is the float32
    rounding of the exact mean, bit-identical run to run and for any batch size or alignment (include/dvmvs_hip.h).  ``out``: a
    contiguous float32 [N,8] tensor (e.g. rows of a larger table), returned; ``counts``: a contiguous int32 [N,4] tensor that receives n
    and the three inlier counts.  Runs on the current stream, without allocation once the workspace of this size exists."""
    check_tensors("depth_errors", gt, label="gt")
    check_tensors("depth_errors", pred, label="pred")
    N, pixels = _frames_2d("depth_errors", gt)
    if _frames_2d("depth_errors", pred) != (N, pixels) or tuple(gt.shape[-2:]) != tuple(pred.shape[-2:]) or gt.device != pred.device:
        raise ValueError(f"dvmvs::depth_errors: gt {tuple(gt.shape)} on {gt.device} and pred {tuple(pred.shape)} on {pred.device} differ")
    if N < 1 or pixels < 1:
        raise ValueError(f"dvmvs::depth_errors: expected non-empty depth maps, got {tuple(gt.shape)}")
    max_depth = float(max_depth)
    if max_depth != max_depth:
        raise ValueError("dvmvs::depth_errors: max_depth is NaN")
    gt, pred = gt.contiguous(), pred.contiguous()
    out = out_or_new("depth_errors", out, (N, 8), torch.float32, gt.device)
    if counts is not None:
        check_tensors("depth_errors", counts, dtype=torch.int32, label="counts", shape=(N, 4), device=gt.device, contiguous=True)
    workspace = depth_errors_workspace(gt.device, N, pixels)
    try:
        launch("dvmvs_depth_errors_fwd", gt.device, ptr(gt), ptr(pred), N, pixels, max_depth, ptr(out), opt_ptr(counts), ptr(workspace))
    except RuntimeError:      # the ticket words may no longer be zero
        _workspace.drop("depth_errors", gt.device, (N, pixels))
        raise
    return out


# ----------------------------------------------------------------------------------------------------------------------
# ray-casting a fused TSDF volume from camera views
# ----------------------------------------------------------------------------------------------------------------------
def _volumes(name, tsdf, weight, color=None):
    """The tensors of a TSDF volume: contiguous float32 [X,Y,Z] on one GPU, every dimension at least 2; returns (X, Y, Z)."""
    check_tensors(name, tsdf, label="tsdf", shape=(None, None, None), contiguous=True)
    X, Y, Z = (int(d) for d in tsdf.shape)
    for label, t in (("weight", weight), ("color", color)):
        if t is not None:
            check_tensors(name, t, label=label, shape=(X, Y, Z), device=tsdf.device, contiguous=True)
    if min(X, Y, Z) < 2:
        raise ValueError(f"dvmvs::{name}: every dimension of the volume must be at least 2, got {X}x{Y}x{Z}")
    return X, Y, Z


def tsdf_raycast_mask(tsdf: Tensor, weight: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """Brick mask of a TSDF volume for ``tsdf_raycast``: uint8 [ceil((X-1)/8), ceil((Y-1)/8), ceil((Z-1)/8)], 1 where one of the brick's
    8x8x8 cells has a corner with ``weight > 0 and tsdf <= 0``.  It describes the volume's CURRENT contents: rebuild it after every
    change.  ``out``: a contiguous uint8 tensor of that shape; it is returned."""
    X, Y, Z = _volumes("tsdf_raycast_mask", tsdf, weight)
    shape = ((X + 6) // 8, (Y + 6) // 8, (Z + 6) // 8)
    nbytes = _capi.lib().dvmvs_tsdf_raycast_mask_bytes(X, Y, Z)
    if nbytes == 0:
        _capi.check(EUNSUPPORTED, "dvmvs_tsdf_raycast_mask_bytes")
    assert nbytes == shape[0] * shape[1] * shape[2]
    out = out_or_new("tsdf_raycast_mask", out, shape, torch.uint8, tsdf.device)
    launch("dvmvs_tsdf_raycast_mask", tsdf.device, ptr(tsdf), ptr(weight), X, Y, Z, ptr(out))
    return out


def tsdf_raycast(tsdf: Tensor, weight: Tensor, color: Optional[Tensor], origin: Sequence[float], voxel_size: float, cam_intr: Tensor,
                 cam_pose: Tensor, height: int, width: int, near: float = 0.0, far: float = float("inf"), step: float = 1.0,
                 mask: Optional[Tensor] = None, normals: bool = True, colour: bool = True):
    """Renders a TSDF volume (the three float32 [X,Y,Z] device tensors of ``dvmvs.tsdf.TSDFVolume``; ``color`` may be None without
    ``colour``) from N views in one launch: ``cam_intr`` [N,3,3] and camera-to-world ``cam_pose`` [N,4,4], float32 on the volume's device.
    Returns ``(depth [N,height,width] float32, normals [N,height,width,3] float32 or None, rgb [N,height,width,3] uint8 or None)``: the
    camera depth of the first zero crossing along each pixel's ray (0 = no surface), the world-space unit normal there (zero where it is
    undefined) and the colour of the nearest voxel.  ``step``: sample spacing in voxels, in (0, 5].  ``mask``: the result of
    ``tsdf_raycast_mask`` for the same volume contents (empty bricks are jumped over; same bits) or None for the dense march.
    Definition: include/dvmvs_hip.h.  Runs on the current stream without touching the host."""
    X, Y, Z = _volumes("tsdf_raycast", tsdf, weight, color)
    dev = tsdf.device
    if colour and color is None:
        raise ValueError("dvmvs::tsdf_raycast: colour output needs the colour volume")
    check_tensors("tsdf_raycast", cam_intr, label="cam_intr", shape=(None, 3, 3), device=dev)
    check_tensors("tsdf_raycast", cam_pose, label="cam_pose", shape=(None, 4, 4), device=dev)
    N = int(cam_pose.shape[0])
    height, width = int(height), int(width)
    if N < 1 or cam_intr.shape[0] != N or height < 1 or width < 1:
        raise ValueError(f"dvmvs::tsdf_raycast: expected N >= 1 poses and as many intrinsics and a positive image size, got "
                         f"{tuple(cam_pose.shape)}, {tuple(cam_intr.shape)}, {height}x{width}")
    near, far, step, voxel_size = float(near), float(far), float(step), float(voxel_size)
    if not (0.0 < step <= 5.0):
        raise ValueError(f"dvmvs::tsdf_raycast: step must be in (0, 5] voxels (the truncation), got {step}")
    if not (0.0 <= near < float("inf")) or far != far:
        raise ValueError(f"dvmvs::tsdf_raycast: near must be finite and >= 0 and far not NaN, got {near}, {far}")
    if not voxel_size > 0.0:
        raise ValueError(f"dvmvs::tsdf_raycast: voxel_size must be positive, got {voxel_size}")
    origin = [float(o) for o in origin]
    if len(origin) != 3:
        raise ValueError("dvmvs::tsdf_raycast: origin must have three components")
    if mask is not None:     # the tensor of tsdf_raycast_mask
        check_tensors("tsdf_raycast", mask, dtype=torch.uint8, label="mask", shape=((X + 6) // 8, (Y + 6) // 8, (Z + 6) // 8), device=dev,
                      contiguous=True)
    cam_intr, cam_pose = cam_intr.contiguous(), cam_pose.contiguous()
    depth = torch.empty((N, height, width), dtype=torch.float32, device=dev)
    normal = torch.empty((N, height, width, 3), dtype=torch.float32, device=dev) if normals else None
    rgb = torch.empty((N, height, width, 3), dtype=torch.uint8, device=dev) if colour else None
    launch("dvmvs_tsdf_raycast_fwd", dev, ptr(tsdf), ptr(weight), opt_ptr(color), X, Y, Z, origin[0], origin[1], origin[2], voxel_size,
           opt_ptr(mask), ptr(cam_intr), ptr(cam_pose), N, height, width, near, far, step, ptr(depth), opt_ptr(normal), opt_ptr(rgb))
    return depth, normal, rgb


# ----------------------------------------------------------------------------------------------------------------------
# fusing a batch of frames into a TSDF volume: one pass over the volume, the bits of per-frame integration
# ----------------------------------------------------------------------------------------------------------------------
# the tile (voxels in x, y, z) one workgroup of csrc/tsdf_fuse.hip takes: kFuseTX, kFuseTY, kFuseTZ there.  Only the tile counters depend on
# it, never the volume.
TSDF_FUSE_TILE = (4, 4, 32)


def tsdf_fuse_tile_count(dims, tile=TSDF_FUSE_TILE):
    """Number of tiles (workgroups) ``tsdf_integrate_frames`` cuts a volume of ``dims`` voxels into."""
    count = 1
    for d, t in zip(dims, tile):
        count *= -(-int(d) // t)
    return count


def tsdf_integrate_frames_workspace(device, n_frames):
    """Persistent workspace of ``tsdf_integrate_frames`` per device: grown to the largest batch seen, written by every call before it is
    read (the per-frame largest depth), so it needs no initialisation; calls that share it must be ordered (one stream per process)."""
    return _workspace.grown("tsdf_fuse", device, _capi.lib().dvmvs_tsdf_integrate_frames_workspace_bytes(n_frames), torch.float32)


def tsdf_integrate_frames(tsdf: Tensor, weight: Tensor, color: Tensor, origin: Sequence[float], voxel_size: float, cam_intr: Tensor,
                          cam_pose: Tensor, depth: Tensor, rgb_u8: Optional[Tensor] = None, folded: Optional[Tensor] = None,
                          trunc_margin: Optional[float] = None, obs_weight=1.0, max_depth: float = float("inf"), stats=False):
    """Fuses N frames into a TSDF volume in place (the three contiguous float32 [X,Y,Z] device tensors of ``dvmvs.tsdf.TSDFVolume``) with
    one pass over the volume and the bits of N ``dvmvs_tsdf_integrate`` calls in frame order (csrc/tsdf_fuse.hip; contract in
    include/dvmvs_hip.h).  ``cam_intr`` [N,3,3], camera-to-world ``cam_pose`` [N,4,4] and ``depth`` [N,h,w] are contiguous float32 tensors on
    the volume's device; the colour is EITHER ``rgb_u8`` [N,h,w,3] uint8 OR ``folded`` [N,h,w] float32 (``dvmvs.tsdf.fold_color``).
    ``trunc_margin`` defaults to 5 voxels; ``obs_weight``: one number or N; a depth above ``max_depth`` counts as invalid.  ``stats``:
    True returns a fresh int64 [2] device tensor holding the (tile, frame) pairs the culling kept and the tiles that loaded the volume;
    a tensor is added to and returned; False (default) returns None and the kernel does not count.  Runs on the current stream without
    touching the host."""
    name = "tsdf_integrate_frames"
    if (rgb_u8 is None) == (folded is None):
        raise ValueError(f"dvmvs::{name}: exactly one of rgb_u8 and folded must be given")
    # every malformed argument is reported before a misplaced one: dtypes and shapes first, devices and contiguity after the scalars
    check_tensors(name, depth, label="depth", shape=(None, None, None), on_gpu=False)
    N, h, w = (int(d) for d in depth.shape)
    if N < 1 or h < 1 or w < 1:
        raise ValueError(f"dvmvs::{name}: expected at least one non-empty frame, got depth {tuple(depth.shape)}")
    check_tensors(name, tsdf, label="tsdf", shape=(None, None, None), on_gpu=False)
    X, Y, Z = (int(d) for d in tsdf.shape)
    if X * Y * Z == 0:
        raise ValueError(f"dvmvs::{name}: tsdf must be a non-empty [X,Y,Z] tensor, got {tuple(tsdf.shape)}")
    checks = [("tsdf", tsdf, torch.float32, (X, Y, Z)), ("weight", weight, torch.float32, (X, Y, Z)), ("color", color, torch.float32, (X, Y, Z)),
              ("cam_intr", cam_intr, torch.float32, (N, 3, 3)), ("cam_pose", cam_pose, torch.float32, (N, 4, 4)),
              ("depth", depth, torch.float32, (N, h, w)),
              ("rgb_u8", rgb_u8, torch.uint8, (N, h, w, 3)) if rgb_u8 is not None else ("folded", folded, torch.float32, (N, h, w))]
    for label, t, dtype, shape in checks:
        check_tensors(name, t, dtype=dtype, label=label, shape=shape, on_gpu=False)
    if hasattr(obs_weight, "tolist"):       # a numpy array or a tensor (one download, not one per element): a 0-d one becomes a number
        obs_weight = obs_weight.tolist()
    weights = [float(x) for x in obs_weight] if isinstance(obs_weight, (list, tuple)) else [float(obs_weight)] * N
    if len(weights) != N:
        raise ValueError(f"dvmvs::{name}: {len(weights)} observation weights for {N} frames")
    voxel_size, max_depth = float(voxel_size), float(max_depth)
    trunc_margin = 5.0 * voxel_size if trunc_margin is None else float(trunc_margin)
    if not voxel_size > 0.0 or not trunc_margin > 0.0 or max_depth != max_depth:
        raise ValueError(f"dvmvs::{name}: voxel_size and trunc_margin must be positive and max_depth not NaN, got "
                         f"{voxel_size}, {trunc_margin}, {max_depth}")
    origin = [float(o) for o in origin]
    if len(origin) != 3:
        raise ValueError(f"dvmvs::{name}: origin must have three components")
    dev = tsdf.device
    for label, t, dtype, shape in checks:
        check_tensors(name, t, dtype=dtype, label=label, shape=shape, device=dev, contiguous=True)
    counters = None
    if torch.is_tensor(stats):
        check_tensors(name, stats, dtype=torch.int64, label="stats", shape=(2,), device=dev, contiguous=True)
        counters = stats
    elif stats:
        counters = torch.zeros(2, dtype=torch.int64, device=dev)
    workspace = tsdf_integrate_frames_workspace(dev, N)
    launch("dvmvs_tsdf_integrate_frames", dev, ptr(tsdf), ptr(weight), ptr(color), X, Y, Z, origin[0], origin[1], origin[2], voxel_size,
           ptr(cam_intr), ptr(cam_pose), opt_ptr(rgb_u8), opt_ptr(folded), ptr(depth), N, h, w, trunc_margin, _capi.float_array(weights),
           max_depth, ptr(workspace), opt_ptr(counters))
    return counters


# ----------------------------------------------------------------------------------------------------------------------
# exact nearest-point distances between point clouds, and the 3-D reconstruction metrics they reduce to
# ----------------------------------------------------------------------------------------------------------------------
def nearest_distance_workspace(device, M):
    """Persistent grid workspace of ``nearest_build`` per device: grown to the largest target cloud seen (its size follows from ``M`` alone)
    and written by every build before a query reads it, so it needs no initialisation.  A build overwrites the grid of the build before
    it: calls that share the workspace must be ordered with respect to each other (one stream per process), and a grid that has to
    outlive the next build needs a buffer of its own (``nearest_build(target, workspace=...)``)."""
    nbytes = _capi.lib().dvmvs_nearest_workspace_bytes(int(M))
    if nbytes == 0:
        raise ValueError(f"dvmvs::nearest_distance: a target cloud of {M} points is outside what the kernels take (1 .. 2^28)")
    return _workspace.grown("nearest_grid", device, nbytes, torch.uint8)


def _points(name, label, t):
    check_tensors(name, t, label=label, shape=(None, 3))
    return t.contiguous()


def nearest_build(target: Tensor, workspace: Optional[Tensor] = None) -> Tensor:
    """Bins ``target`` (float32 [M,3] on the GPU, finite, M >= 1) into a uniform grid over its bounding box (csrc/nearest_points.hip) and
    returns the workspace that holds it, for ``nearest_query``.  The box, the cell edge and the grid's dimensions are computed on the
    device; the host sizes the workspace from M alone.  ``workspace``: a uint8 device tensor of at least
    ``dvmvs_nearest_workspace_bytes(M)`` bytes to build into, instead of the per-device one of ``nearest_distance_workspace``.  Runs on
    the current stream, no synchronisation."""
    target = _points("nearest_build", "target", target)
    M = int(target.shape[0])
    if M < 1:
        raise ValueError("dvmvs::nearest_build: the target cloud is empty")
    if workspace is None:
        workspace = nearest_distance_workspace(target.device, M)
    else:
        check_tensors("nearest_build", workspace, dtype=torch.uint8, label="workspace", device=target.device, contiguous=True)
        if workspace.numel() < _capi.lib().dvmvs_nearest_workspace_bytes(M):
            raise ValueError(f"dvmvs::nearest_build: workspace must have at least {_capi.lib().dvmvs_nearest_workspace_bytes(M)} bytes")
    launch("dvmvs_nearest_build", target.device, ptr(target), M, ptr(workspace), workspace.numel())
    return workspace


def nearest_grid_header(workspace: Tensor) -> dict:
    """The grid a ``nearest_build`` left in ``workspace``, DOWNLOADED (a synchronisation: for tests and tools, not for the hot path):
    ``mn`` and ``mx`` float32 [3] (the targets' box), ``inv_h`` and ``h_lo`` float32, ``dim`` int32 [3], ``ncells``.  A coordinate x falls
    into cell ``int((clamp(x, mn, mx) - mn) * inv_h)`` of its axis, every operation in float32 (include/dvmvs_hip.h)."""
    words = workspace[:48].cpu().numpy()
    floats, ints = words.view(np.float32), words.view(np.int32)
    return {"mn": floats[0:3].copy(), "mx": floats[3:6].copy(), "inv_h": floats[6], "h_lo": floats[7], "dim": ints[8:11].copy(), "ncells": int(ints[11])}


def nearest_query(query: Tensor, target: Tensor, workspace: Tensor, return_index: bool = False):
    """Distances from ``query`` (float32 [N,3]) to the nearest point of ``target``, whose grid ``workspace`` holds (``nearest_build`` of the
    SAME target tensor contents): float32 [N], and with ``return_index`` also int32 [N], the smallest index of a nearest target.  The
    queries are binned in a per-device scratch buffer that every call reuses: like the grid workspace it assumes that the calls of a
    process are ordered with respect to each other (one stream, or streams that wait for each other)."""
    query, target = _points("nearest_query", "query", query), _points("nearest_query", "target", target)
    N, M = int(query.shape[0]), int(target.shape[0])
    if M < 1:
        raise ValueError("dvmvs::nearest_query: the target cloud is empty")
    if query.device != target.device or not torch.is_tensor(workspace) or workspace.device != target.device:
        raise ValueError(f"dvmvs::nearest_query: query, target and workspace must be on one device, got {query.device}, {target.device}")
    dist = torch.empty(N, dtype=torch.float32, device=query.device)
    index = torch.empty(N, dtype=torch.int32, device=query.device) if return_index else None
    if N > 0:
        scratch = _workspace.grown("nearest_query", query.device, _capi.lib().dvmvs_nearest_query_workspace_bytes(N, M), torch.uint8)
        launch("dvmvs_nearest_distance_fwd", query.device, ptr(query), N, ptr(target), M, ptr(workspace), ptr(scratch), scratch.numel(),
               ptr(dist), opt_ptr(index))
    return (dist, index) if return_index else dist


def nearest_distance(query: Tensor, target: Tensor, return_index: bool = False):
    """For every point of ``query`` (float32 [N,3] on the GPU) the exact distance to the nearest point of ``target`` (float32 [M,3], M >= 1):
    float32 [N]; with ``return_index`` also int32 [N], the smallest index of a nearest target.  ``dist[i] = sqrt(min_j (dx*dx + dy*dy) +
    dz*dz)`` with every operation rounded to float32 and no FMA: bit-identical to a brute force over all pairs, run to run, whatever the
    grid prunes (include/dvmvs_hip.h).  Coordinates must be finite (not checked).  One build and one query on the current stream, no
    synchronisation, no allocation once the per-device workspaces have grown to the sizes in use."""
    return nearest_query(query, target, nearest_build(target), return_index)


def distance_metrics(dist_pred: Tensor, dist_gt: Tensor, threshold: float = 0.05, out: Optional[Tensor] = None,
                     counts: Optional[Tensor] = None) -> Tensor:
    """The row (acc, comp, chamfer, precision, recall, fscore) of ``dvmvs.errors.compute_reconstruction_errors`` from the two distance
    arrays: ``dist_pred`` float32 [Na] prediction -> ground truth, ``dist_gt`` float32 [Nb] ground truth -> prediction, both non-empty and
    on the GPU.  Sums in float64 in a fixed order (one workgroup); float32 [6] device tensor (``out`` when given).  ``counts``: a
    contiguous int64 [2] device tensor that receives the numbers of distances below ``threshold``."""
    for label, t in (("dist_pred", dist_pred), ("dist_gt", dist_gt)):
        check_tensors("distance_metrics", t, label=label, shape=(None,))
        if t.numel() < 1:
            raise ValueError(f"dvmvs::distance_metrics: {label} is empty")
    dev = dist_pred.device
    threshold = float(threshold)
    if dist_gt.device != dev or threshold != threshold:
        raise ValueError(f"dvmvs::distance_metrics: both arrays must be on one device and the threshold not NaN, got {dev}, {dist_gt.device}, "
                         f"{threshold}")
    dist_pred, dist_gt = dist_pred.contiguous(), dist_gt.contiguous()
    out = out_or_new("distance_metrics", out, (6,), torch.float32, dev)
    if counts is not None:
        check_tensors("distance_metrics", counts, dtype=torch.int64, label="counts", shape=(2,), device=dev, contiguous=True)
    launch("dvmvs_distance_metrics_fwd", dev, ptr(dist_pred), dist_pred.numel(), ptr(dist_gt), dist_gt.numel(), threshold, ptr(out),
           opt_ptr(counts))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# point sets for the 3-D metrics: area-weighted samples of a triangle mesh, one point per occupied voxel of a cloud
# ----------------------------------------------------------------------------------------------------------------------
_SURFACE_SAMPLE_MAX_POINTS = 1 << 28


def surface_sample(verts: Tensor, faces: Tensor, density: float, seed: int = 0, return_face: bool = False):
    """``dvmvs.errors.sample_surface`` on the device, bit for bit (csrc/surface_sample.hip; definition in include/dvmvs_hip.h): points on
    the triangle mesh ``verts`` float32 [V,3], ``faces`` int32 [F,3] (both on the GPU), about ``density`` per square metre, spread over the
    faces in proportion to their areas: float32 [N,3] in a fixed order (point k depends on k and the mesh alone); with ``return_face``
    also int32 [N], the face of each point.  A face with an index outside [0, V) or without area gets no point, and no vertex is read for
    it.  Four launches on the current stream and ONE host read (a synchronisation) between them: N, to size the output, with the status.
    No points (an empty mesh, or one smaller than half a sample's share of area) gives an empty [0,3] tensor.  Raises ``ValueError`` for a
    density that is not positive, a mesh of 2^31 square metres or more (or with a face whose area is not finite) and N above 2^28."""
    name = "surface_sample"
    check_tensors(name, verts, label="verts", shape=(None, 3))
    check_tensors(name, faces, dtype=torch.int32, label="faces", shape=(None, 3), device=verts.device)
    density, seed = float(density), int(seed)
    if not density > 0.0 or density == float("inf"):
        raise ValueError(f"dvmvs::{name}: density must be positive and finite, got {density}")
    if not 0 <= seed < 2 ** 32:
        raise ValueError(f"dvmvs::{name}: seed must fit 32 unsigned bits, got {seed}")
    dev = verts.device
    verts, faces = verts.contiguous(), faces.contiguous()
    V, F = int(verts.shape[0]), int(faces.shape[0])
    N = 0
    if F > 0:
        nbytes = _capi.lib().dvmvs_surface_sample_workspace_bytes(F)
        if nbytes == 0:
            raise ValueError(f"dvmvs::{name}: a mesh of {F} faces is outside what the kernels take (2^28 at most)")
        workspace = _workspace.grown("surface_sample", dev, nbytes, torch.int64)
        counts = torch.empty(3, dtype=torch.int64, device=dev)
        launch("dvmvs_surface_sample_count", dev, opt_ptr(verts if V else None), V, ptr(faces), F, density, ptr(workspace),
               workspace.numel() * 8, ptr(counts))
        N, status, _ = (int(c) for c in counts.cpu())             # the one host read
        if status != 0:
            raise ValueError(f"dvmvs::{name}: a face's area is not finite or the mesh is larger than 2^31 square metres")
        if N > _SURFACE_SAMPLE_MAX_POINTS:
            raise ValueError(f"dvmvs::{name}: {N} samples are more than 2^28; lower the density")
    points = torch.empty((N, 3), dtype=torch.float32, device=dev)
    face = torch.empty(N, dtype=torch.int32, device=dev) if return_face else None
    if N > 0:
        launch("dvmvs_surface_sample_emit", dev, ptr(verts), V, ptr(faces), F, density, seed, ptr(workspace), N, ptr(points), opt_ptr(face))
    return (points, face) if return_face else points


def voxel_downsample(points: Tensor, voxel: float, return_counts: bool = False):
    """``dvmvs.errors.voxel_down_sample`` on the device, bit for bit (csrc/surface_sample.hip; definition in include/dvmvs_hip.h): one
    point per occupied voxel of edge ``voxel``, the mean of the voxel's points, the voxels in ascending order of their key (x, then y,
    then z cell): float32 [M,3]; with ``return_counts`` also int32 [M], the points per voxel.  ``points``: float32 [N,3] on the GPU,
    finite, N >= 1.  The cells are counted from the cloud's own minimum; a voxel's sum runs in float64 over its points in ascending
    index.  Seven launches and a stable ``torch.sort`` of the keys on the current stream, and ONE host read (a synchronisation): M, to
    size the output, with the status.  Linear in N whatever the voxels' populations.  Raises ``ValueError`` for an empty cloud, a voxel
    that is not positive, and a cloud that spans 2^21 voxels or more on an axis."""
    name = "voxel_downsample"
    check_tensors(name, points, label="points", shape=(None, 3))
    voxel = float(voxel)
    if not voxel > 0.0 or voxel == float("inf"):
        raise ValueError(f"dvmvs::{name}: voxel must be positive and finite, got {voxel}")
    inv = float(np.float32(1.0 / voxel))
    if not 0.0 < inv < float("inf"):
        raise ValueError(f"dvmvs::{name}: 1 / voxel is not a positive float32 for voxel {voxel}")
    dev = points.device
    points = points.contiguous()
    N = int(points.shape[0])
    if N < 1:
        raise ValueError(f"dvmvs::{name}: the cloud is empty")
    nbytes = _capi.lib().dvmvs_voxel_downsample_workspace_bytes(N)
    if nbytes == 0:
        raise ValueError(f"dvmvs::{name}: a cloud of {N} points is outside what the kernels take (2^28 at most)")
    workspace = _workspace.grown("voxel_downsample", dev, nbytes, torch.uint8)
    keys = torch.empty(N, dtype=torch.int64, device=dev)
    launch("dvmvs_voxel_keys", dev, ptr(points), N, inv, ptr(workspace), workspace.numel(), ptr(keys))
    sorted_keys, sorted_index = torch.sort(keys, stable=True)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    launch("dvmvs_voxel_downsample_count", dev, ptr(points), N, ptr(sorted_keys), ptr(sorted_index), ptr(workspace), workspace.numel(),
           ptr(counts))
    M, status = (int(c) for c in counts.cpu())                    # the one host read
    if status != 0:
        raise ValueError(f"dvmvs::{name}: the cloud spans 2^21 voxels or more on an axis (or holds a coordinate that is not finite)")
    out = torch.empty((M, 3), dtype=torch.float32, device=dev)
    population = torch.empty(M, dtype=torch.int32, device=dev) if return_counts else None
    launch("dvmvs_voxel_downsample_emit", dev, N, M, ptr(workspace), ptr(out), opt_ptr(population))
    return (out, population) if return_counts else out


# ----------------------------------------------------------------------------------------------------------------------
# rasterising a triangle mesh to depth maps, and the vertices that depth maps show
# ----------------------------------------------------------------------------------------------------------------------
# a clipped triangle whose box of candidate pixels holds more pixels than this goes to the device work list (one pixel per lane) instead
# of being rasterised by the thread of its (view, face): DVMVS_MESH_RASTER_LARGE_BOX in include/dvmvs_hip.h.  It cannot change a result.
MESH_RASTER_LARGE_BOX = 64
MESH_RASTER_TILE = 16             # the edge of a list entry's tile of the image grid (kMrTile in csrc/mesh_raster.hip)


def mesh_raster_cameras(cam_poses: Tensor) -> Tensor:
    """World-to-camera matrices [N,3,4] float32 of camera-to-world poses float32 [N,4,4] on the GPU, as ``mesh_raster`` and
    ``mesh_visibility`` use them: the inverse in float64 on the device, rounded once (``dvmvs_mesh_raster_cameras``: one tiny launch;
    the same as a chain of small torch operations took 0.07 ms, more than the rest of a
    ``mesh_raster`` call on a 190 000-face mesh).  No host read, no synchronisation."""
    check_tensors("mesh_raster_cameras", cam_poses, label="cam_poses", shape=(None, 4, 4))
    N = int(cam_poses.shape[0])
    w2c = torch.empty((N, 3, 4), dtype=torch.float32, device=cam_poses.device)
    if N > 0:
        launch("dvmvs_mesh_raster_cameras", cam_poses.device, ptr(cam_poses.contiguous()), ptr(w2c), N)
    return w2c


def _mesh_cameras(name, cam_intr, cam_poses, dev):
    check_tensors(name, cam_intr, label="cam_intr", shape=(None, 3, 3), device=dev)
    check_tensors(name, cam_poses, label="cam_poses", shape=(None, 4, 4), device=dev)
    N = int(cam_poses.shape[0])
    if N < 1 or N > 65535 or cam_intr.shape[0] != N:
        raise ValueError(f"dvmvs::{name}: expected 1 .. 65535 poses and as many intrinsics, got {tuple(cam_poses.shape)} and {tuple(cam_intr.shape)}")
    return N, cam_intr.contiguous(), mesh_raster_cameras(cam_poses)


def _mesh_near(name, near):
    near = float(near)
    if not 0.0 < near < float("inf"):
        raise ValueError(f"dvmvs::{name}: near must be positive and finite, got {near}")
    return near


def mesh_raster_workspace_bytes(n_views, n_faces, height, width):
    """Bytes of workspace ``mesh_raster`` needs for the shape (host arithmetic); raises ``ValueError`` for a shape the kernels refuse."""
    nbytes = _capi.lib().dvmvs_mesh_raster_workspace_bytes(int(n_views), int(n_faces), int(height), int(width))
    if nbytes == 0:
        raise ValueError(f"dvmvs::mesh_raster: {n_views} views of {height}x{width} pixels of {n_faces} faces are outside what the kernels take "
                         f"(1 .. 65535 views, 1 .. 2^28 faces, sides up to 16384, fewer than 2^31 pixels in all)")
    return nbytes


def mesh_raster_workspace(device, n_views, n_faces, height, width):
    """Persistent workspace of ``mesh_raster`` per device: grown to the largest shape seen; every call writes what it reads first (the
    z-buffer keys, the work list's length), so it needs no initialisation.  Calls that share it must be ordered (one stream per process)."""
    return _workspace.grown("mesh_raster", device, mesh_raster_workspace_bytes(n_views, n_faces, height, width), torch.int64)


def mesh_raster(verts: Tensor, faces: Tensor, cam_intr: Tensor, cam_poses: Tensor, height: int, width: int, near: float = 0.05,
                far: float = float("inf"), cull_backfaces: bool = False, workspace: Optional[Tensor] = None, return_overflow: bool = False,
                large_box: Optional[int] = None):
    """Rasterises the triangle mesh ``verts`` float32 [V,3] (world space), ``faces`` int32 [F,3] from N views in one call
    (csrc/mesh_raster.hip; definition in include/dvmvs_hip.h): ``cam_intr`` float32 [N,3,3], camera-to-world ``cam_poses`` float32 [N,4,4],
    all on one GPU.  Returns ``(depth [N,height,width] float32, face [N,height,width] int32)``: the camera depth of the nearest face at
    every pixel (0 where there is none between ``near`` and ``far``) and that face's index (-1); with ``return_overflow`` also int32 [N],
    the clipped triangles per view that were left out because a corner projects beyond 2^21 pixels.  Pixels are sampled at their integer
    coordinates, as ``tsdf_raycast`` does.  A face that crosses ``z = near`` is clipped; at equal depths the lowest face index wins; the
    result does not depend on the order of the faces or on ``large_box`` (the tuning constant ``MESH_RASTER_LARGE_BOX``).  ``workspace``:
    an int64 device tensor of at least ``mesh_raster_workspace_bytes(N, F, height, width)`` bytes, of any contents, instead of the
    per-device one.  An empty mesh gives empty maps.  Runs on the current stream: no host read and no synchronisation."""
    name = "mesh_raster"
    check_tensors(name, verts, label="verts", shape=(None, 3))
    dev = verts.device
    check_tensors(name, faces, dtype=torch.int32, label="faces", shape=(None, 3), device=dev)
    N, K, w2c = _mesh_cameras(name, cam_intr, cam_poses, dev)
    height, width, near, far = int(height), int(width), _mesh_near(name, near), float(far)
    if height < 1 or width < 1 or far != far:
        raise ValueError(f"dvmvs::{name}: expected a positive image size and a far that is a number, got {height}x{width}, {far}")
    large_box = MESH_RASTER_LARGE_BOX if large_box is None else int(large_box)
    if large_box < 1:
        raise ValueError(f"dvmvs::{name}: large_box must be at least 1, got {large_box}")
    V, F = int(verts.shape[0]), int(faces.shape[0])
    nbytes = mesh_raster_workspace_bytes(N, max(F, 1), height, width)
    if workspace is not None:
        check_tensors(name, workspace, dtype=torch.int64, label="workspace", shape=(None,), device=dev, contiguous=True)
        if workspace.numel() * 8 < nbytes:
            raise ValueError(f"dvmvs::{name}: workspace must have at least {nbytes} bytes, got {workspace.numel() * 8}")
    if V == 0 or F == 0:
        depth = torch.zeros((N, height, width), dtype=torch.float32, device=dev)
        face = torch.full((N, height, width), -1, dtype=torch.int32, device=dev)
        overflow = torch.zeros(N, dtype=torch.int32, device=dev)
        return (depth, face, overflow) if return_overflow else (depth, face)
    if workspace is None:
        workspace = mesh_raster_workspace(dev, N, F, height, width)
    verts, faces = verts.contiguous(), faces.contiguous()
    depth = torch.empty((N, height, width), dtype=torch.float32, device=dev)
    face = torch.empty((N, height, width), dtype=torch.int32, device=dev)
    overflow = torch.empty(N, dtype=torch.int32, device=dev)
    launch("dvmvs_mesh_raster_fwd", dev, ptr(verts), V, ptr(faces), F, ptr(K), ptr(w2c), N, height, width, near, far, 1 if cull_backfaces else 0,
           large_box, ptr(workspace), workspace.numel() * 8, ptr(depth), ptr(face), ptr(overflow))
    return (depth, face, overflow) if return_overflow else (depth, face)


def mesh_visibility(verts: Tensor, depth: Tensor, cam_intr: Tensor, cam_poses: Tensor, near: float = 0.05, relative: float = 0.01,
                    absolute: float = 0.0) -> Tensor:
    """For every vertex of ``verts`` float32 [V,3] the number of views that see it, int32 [V] (definition in include/dvmvs_hip.h): view r
    sees a vertex whose camera depth z is at least ``near``, whose projection lies inside the image, and with
    ``z <= D (1 + relative) + absolute`` for the largest positive ``D`` among the up to four pixels of ``depth[r]`` around the projection.
    ``depth`` float32 [N,H,W] (normally ``mesh_raster``'s), ``cam_intr`` [N,3,3], camera-to-world ``cam_poses`` [N,4,4], all on one GPU.
    One launch on the current stream: no host read and no synchronisation."""
    name = "mesh_visibility"
    check_tensors(name, verts, label="verts", shape=(None, 3))
    dev = verts.device
    check_tensors(name, depth, label="depth", shape=(None, None, None), device=dev)
    N, K, w2c = _mesh_cameras(name, cam_intr, cam_poses, dev)
    H, W = int(depth.shape[1]), int(depth.shape[2])
    near, relative, absolute = _mesh_near(name, near), float(relative), float(absolute)
    if depth.shape[0] != N or H < 1 or W < 1:
        raise ValueError(f"dvmvs::{name}: expected {N} non-empty depth maps, got {tuple(depth.shape)}")
    if relative != relative or absolute != absolute:
        raise ValueError(f"dvmvs::{name}: a threshold is NaN")
    mesh_raster_workspace_bytes(N, 1, H, W)          # the shape limits of the family
    V = int(verts.shape[0])
    count = torch.empty(V, dtype=torch.int32, device=dev)
    if V > 0:
        launch("dvmvs_mesh_visibility_fwd", dev, ptr(verts.contiguous()), V, ptr(depth.contiguous()), ptr(K), ptr(w2c), N, H, W, near, relative,
               absolute, ptr(count))
    return count


# ----------------------------------------------------------------------------------------------------------------------
# filtering depth maps by multi-view geometric consistency
# ----------------------------------------------------------------------------------------------------------------------
CONSISTENCY_MAX_SOURCES = 16


def _consistency_cameras(name, K, poses, sources):
    """Checks types and shapes of the camera tensors of the two consistency ops, wherever they are; returns (N, S)."""
    check_tensors(name, K, label="K", shape=(None, 3, 3), on_gpu=False)
    N = int(K.shape[0])
    check_tensors(name, poses, label="poses", shape=(N, 4, 4), on_gpu=False)       # camera-to-world
    check_tensors(name, sources, dtype=torch.int32, label="sources", shape=(N, None), on_gpu=False)
    if N < 1 or N > 65535 or sources.shape[1] > CONSISTENCY_MAX_SOURCES:
        raise ValueError(f"dvmvs::{name}: expected 1 .. 65535 frames and at most {CONSISTENCY_MAX_SOURCES} sources per frame, got K "
                         f"{tuple(K.shape)} and sources {tuple(sources.shape)}")
    return N, int(sources.shape[1])


def _consistency_devices(name, **tensors):
    """Every tensor on the GPU, and on the same one."""
    first = None
    for label, t in tensors.items():
        first = t.device if first is None else first
        check_tensors(name, t, dtype=t.dtype, label=label, device=first)


def consistency_matrices(K: Tensor, poses: Tensor, sources: Tensor) -> Tensor:
    """Step A of the consistency filter (``dvmvs_consistency_matrices``; definition in include/dvmvs_hip.h): for every (frame r, slot j) the
    float32 (A, b) that take a pixel of r and its depth into source ``sources[r][j]``, and (A', b') for the way back, from float64
    arithmetic on the device.  ``K`` float32 [N,3,3], camera-to-world ``poses`` float32 [N,4,4], ``sources`` int32 [N,S] (S <= 16), all on
    the GPU -> float32 [N,S,2,12]; a skipped slot (negative, >= N or the frame itself) holds zeros.  One tiny launch on the current stream."""
    N, S = _consistency_cameras("consistency_matrices", K, poses, sources)
    _consistency_devices("consistency_matrices", K=K, poses=poses, sources=sources)
    K, poses, sources = K.contiguous(), poses.contiguous(), sources.contiguous()
    out = torch.empty((N, S, 2, 12), dtype=torch.float32, device=K.device)
    if S == 0:
        return out
    launch("dvmvs_consistency_matrices", K.device, ptr(K), ptr(poses), ptr(sources), ptr(out), N, S)
    return out


def depth_consistency(depths: Tensor, K: Tensor, poses: Tensor, sources: Tensor, pixel_threshold: float = 1.0,
                      relative_threshold: float = 0.01, min_views: int = 2, average: bool = True, with_count: bool = True,
                      with_points: bool = False, matrices: Optional[Tensor] = None, out: Optional[Tensor] = None):
    """Filters N depth maps by multi-view geometric consistency in one launch (csrc/depth_consistency.hip; definition in
    include/dvmvs_hip.h): a pixel of frame r is projected into each source ``sources[r][j]``, that map is sampled there, the sample is
    projected back, and the source agrees when the pixel returns within ``pixel_threshold`` pixels and ``relative_threshold`` of its depth.
    ``depths`` float32 [N,H,W], ``K`` float32 [N,3,3], camera-to-world ``poses`` float32 [N,4,4], ``sources`` int32 [N,S], all on one GPU.
    Returns ``(depth, count or None, points or None)``: ``depth`` float32 [N,H,W], 0 where fewer than ``min_views`` sources agree and the
    pixel's own depth (``average=False``) or the mean of it and the agreeing re-projections elsewhere; ``count`` uint8 [N,H,W];
    ``points`` float32 [N,H,W,3], the kept pixels in world space (zeros elsewhere).  ``matrices``: ``consistency_matrices(K, poses,
    sources)`` when the caller already has it (saves that launch); ``out``: a contiguous float32 [N,H,W] tensor for ``depth``, e.g. a
    view that starts anywhere inside a larger buffer (must not overlap ``depths``).  Runs on the current stream; no host read and
    no synchronisation."""
    name = "depth_consistency"
    N, S = _consistency_cameras(name, K, poses, sources)
    check_tensors(name, depths, label="depths", shape=(N, None, None), on_gpu=False)
    H, W = int(depths.shape[1]), int(depths.shape[2])
    if H < 1 or W < 1:
        raise ValueError(f"dvmvs::{name}: depths must be non-empty, got {tuple(depths.shape)}")
    if 3 * H * W >= 2 ** 31:
        raise ValueError(f"dvmvs::{name}: a {H}x{W} map is too large (3 H W must stay below 2^31)")
    pixel_threshold, relative_threshold, min_views = float(pixel_threshold), float(relative_threshold), int(min_views)
    if pixel_threshold != pixel_threshold or relative_threshold != relative_threshold:
        raise ValueError(f"dvmvs::{name}: a threshold is NaN")
    if min_views < 0:
        raise ValueError(f"dvmvs::{name}: min_views must not be negative, got {min_views}")
    _consistency_devices(name, depths=depths, K=K, poses=poses, sources=sources)
    dev = depths.device
    if matrices is None:
        matrices = consistency_matrices(K, poses, sources)
    else:     # the tensor of consistency_matrices
        check_tensors(name, matrices, label="matrices", shape=(N, S, 2, 12), device=dev, contiguous=True)
    out = out_or_new(name, out, (N, H, W), torch.float32, dev)
    depths, K, poses, sources = depths.contiguous(), K.contiguous(), poses.contiguous(), sources.contiguous()
    count = torch.empty((N, H, W), dtype=torch.uint8, device=dev) if with_count else None
    points = torch.empty((N, H, W, 3), dtype=torch.float32, device=dev) if with_points else None
    launch("dvmvs_depth_consistency_fwd", dev, ptr(depths), ptr(K), ptr(poses), ptr(sources), ptr(matrices), ptr(out), opt_ptr(count),
           opt_ptr(points), N, S, H, W, pixel_threshold, relative_threshold, min_views, 1 if average else 0)
    return out, count, points

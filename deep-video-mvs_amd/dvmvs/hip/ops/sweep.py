"""The fused plane-sweep cost volume: forward and backward, its host-made plan and work list, its spill workspace, and the "exact"
fp64 pose algebra on the device (the default path is dvmvs.pose_algebra's host fp32)."""
import os
from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from dvmvs.hip import _capi
from dvmvs.hip.ops import _workspace
from dvmvs.hip.ops._common import check_tensors, custom_op, launch, opt_ptr, ptr

# two-pass tiled sweep (spill list in the workspace): see dvmvs_cost_volume_workspace_bytes_two_pass in the header.  Read at call time.
COST_VOLUME_TWO_PASS = os.environ.get("DVMVS_COST_VOLUME_TWO_PASS", "1") == "1"


def sweep_workspace(device, B, M, H, W, D):
    """Persistent spill workspace of the two-pass sweep for (device, shape): zero-filled once here and left zeroed by every
    call (contract in include/dvmvs_hip.h).  Returns (tensor, bytes).

    One buffer per device and shape: calls that use it must be ordered with respect to each other, which is the case for
    the one-process-per-GPU, one-stream-per-process model of this package (a hipGraph replay runs on the stream that
    launches it).  Code that issues cost volumes of the same shape on several streams concurrently must pass its own
    workspaces through the C ABI.  Allocated outside any graph capture when the first (eager / warm-up) call happens."""
    nbytes = _capi.lib().dvmvs_cost_volume_workspace_bytes(B, M, H, W, D)
    return _workspace.zeroed("sweep", device, (B, M, H, W, D), nbytes, torch.float32), nbytes


def drop_sweep_workspace(device, B, M, H, W, D):
    """Forgets the cached workspace of (device, shape).  Called when a cost-volume call fails: its contract (header words zero
    between calls) may no longer hold, and a stale group count would silently corrupt every later volume of that shape."""
    _workspace.drop("sweep", device, (B, M, H, W, D))


def _check_sweep_matrices(name, Hm, kt, B, M):
    if tuple(Hm.shape) != (B, M, 9) or tuple(kt.shape) != (B, M, 3):
        raise ValueError(f"dvmvs::{name}: expected Hm [{B},{M},9] and kt [{B},{M},3] (dvmvs.pose_algebra.sweep_matrices), "
                         f"got {tuple(Hm.shape)} and {tuple(kt.shape)}")


def sweep_work_list_words(B: int, H: int, W: int, D: int) -> int:
    """32-bit words of a sweep work list for this shape (dvmvs_sweep_work_list_bytes / 4)."""
    return int(_capi.lib().dvmvs_sweep_work_list_bytes(int(B), int(H), int(W), int(D))) // 4


def _host_matrices(name, Hm, kt):
    Hm, kt = Hm.contiguous(), kt.contiguous()
    if Hm.device.type != "cpu" or Hm.dtype != torch.float32 or kt.dtype != torch.float32:
        raise ValueError(f"{name} needs the float32 HOST copies of the sweep matrices")
    return Hm, kt


def _check_host_work_list(out, words):
    if out.device.type != "cpu" or out.dtype != torch.int32 or out.numel() < words or not out.is_contiguous():
        raise ValueError(f"work list buffer must be a contiguous int32 host tensor of at least {words} words (sweep_work_list_words)")


def sweep_work_list_host(Hm: Tensor, kt: Tensor, H: int, W: int, D: int, min_depth: float, max_depth: float, variant: int, out: Optional[Tensor] = None):
    """The tiled sweep's work list for HOST matrices ``Hm`` [B,M,9] / ``kt`` [B,M,3] (dvmvs_sweep_work_list: (tile, chunk) pairs whose
    sample boxes had to be halved are cut into plane sub-ranges that separate workgroups process in parallel), as an int32 host tensor
    (``out``: a caller-owned one, e.g. a slice of pinned staging memory).  ``variant``: the launch's (3 = wide configuration)."""
    Hm, kt = _host_matrices("sweep_work_list_host", Hm, kt)
    B, M = Hm.shape[0], Hm.shape[1]
    words = sweep_work_list_words(B, H, W, D)
    if out is None:
        out = torch.empty(words, dtype=torch.int32)
    _check_host_work_list(out, words)
    used = _capi.lib().dvmvs_sweep_work_list(Hm.data_ptr(), kt.data_ptr(), B, M, int(H), int(W), int(D), float(min_depth), float(max_depth),
                                             1 if variant in (3, 5) else 0, out.data_ptr(), out.numel() * 4)
    if used < 0:      # a host walk, not a launch: a non-negative return is the number of bytes used
        _capi.check(used, "dvmvs_sweep_work_list")
    return out


def sweep_plan_host(Hm: Tensor, kt: Tensor, H: int, W: int, D: int, min_depth: float, max_depth: float, variant: int, out: Tensor,
                    allow_mfma: bool = False) -> int:
    """Configuration choice (``variant`` 0; or 2 / 3 as given) and work list in one walk (dvmvs_sweep_plan): fills ``out`` (an int32 host
    tensor of ``sweep_work_list_words``) and returns the variant to launch with."""
    Hm, kt = _host_matrices("sweep_plan_host", Hm, kt)
    _check_host_work_list(out, sweep_work_list_words(Hm.shape[0], H, W, D))
    if allow_mfma and int(variant) == 0:
        # ... with variant 6 (the correlate-then-interpolate sweep) as a candidate: for callers with 32-channel channels-last measurement maps
        chosen = _capi.lib().dvmvs_sweep_plan6(Hm.data_ptr(), kt.data_ptr(), Hm.shape[0], Hm.shape[1], int(H), int(W), int(D), float(min_depth),
                                               float(max_depth), out.data_ptr(), out.numel() * 4)
    else:
        chosen = _capi.lib().dvmvs_sweep_plan(Hm.data_ptr(), kt.data_ptr(), Hm.shape[0], Hm.shape[1], int(H), int(W), int(D), float(min_depth),
                                              float(max_depth), {4: 2, 5: 3}.get(int(variant), int(variant)), out.data_ptr(), out.numel() * 4)
    if chosen < 0:    # a host walk, not a launch: a non-negative return is the variant
        _capi.check(chosen, "dvmvs_sweep_plan")
    return chosen


def _planned_sweep(image1, image2s, Hm, kt, dst, D, min_depth, max_depth, dot_product, variant, nhwc, work_list):
    """dvmvs_cost_volume_planned_fwd into ``dst`` for checked, laid-out inputs; a failed call forgets the spill workspace it used."""
    B, C, H, W = image1.shape
    M = len(image2s)
    workspace, ws_bytes = sweep_workspace(image1.device, B, M, H, W, D) if COST_VOLUME_TWO_PASS else (None, 0)
    if work_list is not None:
        if work_list.device != image1.device or work_list.dtype != torch.int32 or not work_list.is_contiguous() or \
                work_list.numel() < sweep_work_list_words(B, H, W, D):
            raise ValueError("dvmvs::cost_volume: work_list must be a contiguous int32 tensor of dvmvs_sweep_work_list_bytes on the features' device")
    try:
        launch("dvmvs_cost_volume_planned_fwd", image1.device,
               ptr(image1), _capi.pointer_array([ptr(t) for t in image2s]), ptr(Hm), ptr(kt), ptr(dst), B, M, C, H, W, D,
               float(min_depth), float(max_depth), int(bool(dot_product)), int(variant), _capi.LAYOUT_NHWC if nhwc else _capi.LAYOUT_NCHW,
               opt_ptr(workspace), ws_bytes, opt_ptr(work_list))
    except RuntimeError:
        if workspace is not None:
            drop_sweep_workspace(image1.device, B, M, H, W, D)
        raise
    return dst


def cost_volume(image1: Tensor, image2s: Sequence[Tensor], Hm: Tensor, kt: Tensor, min_depth: float, max_depth: float, n_depth_levels: int,
                dot_product: bool, variant: int, work_list: Optional[Tensor] = None) -> Tensor:
    """``Hm`` [B,M,9] = K R K^-1 and ``kt`` [B,M,3] = K t per (batch item, measurement frame): dvmvs.pose_algebra.  ``work_list``: the
    device copy of ``sweep_work_list_host``'s result for these matrices (optional; the tiled sweep then cuts long workgroups).
    Differentiable in the feature maps (dot-product mode)."""
    if work_list is None:      # (the registered op takes a tensor: an empty one = no list)
        work_list = torch.empty(0, dtype=torch.int32, device=image1.device)
    return _cost_volume_op(image1, image2s, Hm, kt, min_depth, max_depth, n_depth_levels, dot_product, variant, work_list)


def _cost_volume_fake(image1, image2s, Hm, kt, min_depth, max_depth, n_depth_levels, dot_product, variant, work_list):
    B, C, H, W = image1.shape
    return image1.new_empty((B, n_depth_levels, H, W))


@custom_op("cost_volume", fake=_cost_volume_fake)
def _cost_volume_op(image1: Tensor, image2s: Sequence[Tensor], Hm: Tensor, kt: Tensor,
                    min_depth: float, max_depth: float, n_depth_levels: int, dot_product: bool, variant: int, work_list: Tensor) -> Tensor:
    check_tensors("cost_volume", image1, Hm, kt, *image2s)
    M = len(image2s)
    if M == 0:
        raise ValueError("dvmvs::cost_volume: need at least one measurement feature map")
    B, C, H, W = image1.shape
    _check_sweep_matrices("cost_volume", Hm, kt, B, M)
    for t in image2s:
        if t.shape != image1.shape:
            raise ValueError(f"dvmvs::cost_volume: measurement features {tuple(t.shape)} != reference {tuple(image1.shape)}")
    image1 = image1.contiguous()
    # Measurement maps that are already channels-last in memory (the frame engine caches them that way) are passed as NHWC;
    # anything else is made NCHW-contiguous, the reference's layout.
    nhwc_ok = bool(dot_product) and variant != 1 and C % 4 == 0 and C > 1 and (H * W >= 64 * 64 or (variant in (6, 7) and C <= 32))
    nhwc = nhwc_ok and all(t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous() for t in image2s)
    image2s = list(image2s) if nhwc else [t.contiguous() for t in image2s]
    out = torch.empty((B, n_depth_levels, H, W), dtype=torch.float32, device=image1.device)
    return _planned_sweep(image1, image2s, Hm.contiguous(), kt.contiguous(), out, n_depth_levels, min_depth, max_depth, dot_product, variant, nhwc,
                          work_list if work_list.numel() else None)


def _cost_volume_setup(ctx, inputs, output):
    image1, image2s, Hm, kt, min_depth, max_depth, n_depth_levels, dot_product, variant = inputs[:9]
    if not dot_product and (image1.requires_grad or any(t.requires_grad for t in image2s)):
        raise NotImplementedError("dvmvs::cost_volume: gradients are implemented for dot_product=True only")
    ctx.M = len(image2s)
    ctx.depth_range = (min_depth, max_depth, n_depth_levels)
    ctx.save_for_backward(image1, Hm, kt, *image2s)


def _cost_volume_backward(ctx, grad):
    saved = ctx.saved_tensors
    M = ctx.M
    image1, Hm, kt = saved[0], saved[1], saved[2]
    image2s = list(saved[3:3 + M])
    min_depth, max_depth, D = ctx.depth_range
    grad = grad.contiguous()
    B, C, H, W = image1.shape
    image1c = image1.contiguous()
    image2c = [t.contiguous() for t in image2s]
    g1 = torch.empty_like(image1c)
    flags = ctx.needs_input_grad[1]   # a tensor-list input: one flag per measurement map
    need2 = any(flags) if isinstance(flags, (list, tuple)) else bool(flags)
    g2 = [torch.zeros_like(t) for t in image2c] if need2 else []
    launch("dvmvs_cost_volume_bwd", image1.device,
           ptr(grad), ptr(image1c), _capi.pointer_array([ptr(t) for t in image2c]), ptr(Hm.contiguous()), ptr(kt.contiguous()),
           ptr(g1), _capi.pointer_array([ptr(t) for t in g2] if need2 else [None] * M),
           B, M, C, H, W, D, float(min_depth), float(max_depth))
    return g1, (g2 if need2 else [None] * M), None, None, None, None, None, None, None, None


torch.library.register_autograd("dvmvs::cost_volume", _cost_volume_backward, setup_context=_cost_volume_setup)


def cost_volume_into(image1: Tensor, image2s, Hm: Tensor, kt: Tensor, min_depth: float, max_depth: float, dst: Tensor, variant: int = 0,
                     work_list: Optional[Tensor] = None) -> Tensor:
    """Dot-product cost volume written into ``dst`` [B,D,H,W] (contiguous: for B == 1 a channel slice of a larger buffer is)."""
    check_tensors("cost_volume_into", image1, Hm, kt, dst, *image2s)
    B, C, H, W = image1.shape
    D = dst.shape[1]
    _check_sweep_matrices("cost_volume_into", Hm, kt, B, len(image2s))
    nhwc = C > 1 and all(t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous() for t in image2s)
    if not (image1.is_contiguous() and dst.is_contiguous() and tuple(dst.shape) == (B, D, H, W) and (nhwc or all(t.is_contiguous() for t in image2s))):
        raise ValueError("dvmvs::cost_volume_into: expected contiguous NCHW tensors (measurement maps: all NCHW or all channels-last)")
    return _planned_sweep(image1, image2s, Hm.contiguous(), kt.contiguous(), dst, D, min_depth, max_depth, True, variant, nhwc, work_list)


def nchw_to_nhwc_into(src: Tensor, dst: Tensor) -> Tensor:
    """``dst`` (a channels-last [B,C,H,W] tensor) = ``src`` (contiguous NCHW), one HIP launch (dvmvs_nchw_to_nhwc: C <= 64, a multiple of 4)."""
    check_tensors("nchw_to_nhwc_into", src, dst)
    B, C, H, W = src.shape
    if tuple(dst.shape) != (B, C, H, W) or not src.is_contiguous() or not dst.is_contiguous(memory_format=torch.channels_last):
        raise ValueError("dvmvs::nchw_to_nhwc_into: expected a contiguous NCHW source and a channels-last destination of the same shape")
    launch("dvmvs_nchw_to_nhwc", src.device, ptr(src), ptr(dst), B, C, H, W)
    return dst


def _sweep_matrices_fake(pose1, pose2s, K):
    B, M = pose1.shape[0], len(pose2s)
    return pose1.new_empty((B, M, 9)), pose1.new_empty((B, M, 3))


@custom_op("sweep_matrices", fake=_sweep_matrices_fake)
def sweep_matrices(pose1: Tensor, pose2s: Sequence[Tensor], K: Tensor) -> Tuple[Tensor, Tensor]:
    """"exact" pose algebra: (Hm [B,M,9], kt [B,M,3]) in fp64 on the device, rounded once (dvmvs_sweep_matrices)."""
    check_tensors("sweep_matrices", pose1, K, *pose2s)
    B, M = pose1.shape[0], len(pose2s)
    if M == 0 or tuple(pose1.shape) != (B, 4, 4) or tuple(K.shape) != (B, 3, 3) or any(tuple(p.shape) != (B, 4, 4) for p in pose2s):
        raise ValueError("dvmvs::sweep_matrices: expected pose1 [B,4,4], M >= 1 measurement poses [B,4,4] and K [B,3,3]")
    pose1, K = pose1.contiguous(), K.contiguous()
    pose2s = [p.contiguous() for p in pose2s]
    Hm = torch.empty((B, M, 9), dtype=torch.float32, device=pose1.device)
    kt = torch.empty((B, M, 3), dtype=torch.float32, device=pose1.device)
    launch("dvmvs_sweep_matrices", pose1.device, ptr(pose1), _capi.pointer_array([ptr(p) for p in pose2s]), ptr(K), ptr(Hm), ptr(kt), B, M)
    return Hm, kt


# inverse(a) @ c for [B,4,4] poses in fp64 on the device, rounded once
@custom_op("relative_pose", fake=lambda a, c: torch.empty_like(a))
def relative_pose(a: Tensor, c: Tensor) -> Tensor:
    check_tensors("relative_pose", a, c)
    if a.shape != c.shape or a.shape[-2:] != (4, 4) or a.dim() != 3:
        raise ValueError(f"dvmvs::relative_pose: expected two [B,4,4] tensors, got {tuple(a.shape)} and {tuple(c.shape)}")
    a, c = a.contiguous(), c.contiguous()
    out = torch.empty_like(a)
    launch("dvmvs_relative_pose", a.device, ptr(a), ptr(c), ptr(out), a.shape[0])
    return out

"""``torch.library`` custom ops over the C ABI of ``libdvmvs_hip.so``.

Each op is a thin shim: check device/dtype, make inputs contiguous, allocate the output with torch, pass raw device
pointers and the current HIP stream to the ``extern "C"`` launcher.  No op synchronises or touches the host, so a
whole frame can be captured into a hipGraph (``torch.cuda.graph``).  Tensors that are not on the GPU are rejected:
the CPU restatement lives in ``oracle/`` and is test infrastructure only.
"""
import ctypes
import os
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from dvmvs.hip import _capi

__all__ = ["cost_volume", "sweep_matrices", "hidden_warp", "relative_pose", "lstm_gates", "depth_reproject", "depth_reproject_lowres",
           "bias_act_", "upsample2x", "depthwise_conv", "rgb_sweep", "gp_filter_step", "dps_volume", "dps_regress", "preprocess_rgb",
           "preprocess_depth", "depth_errors", "tsdf_raycast", "tsdf_raycast_mask", "tsdf_integrate_frames", "nearest_distance", "nearest_build",
           "nearest_query", "distance_metrics", "consistency_matrices", "depth_consistency"]


# two-pass tiled sweep (spill list in the workspace): see dvmvs_cost_volume_workspace_bytes_two_pass in the header
COST_VOLUME_TWO_PASS = os.environ.get("DVMVS_COST_VOLUME_TWO_PASS", "1") == "1"


_workspaces = {}


def sweep_workspace(device, B, M, H, W, D):
    """Persistent spill workspace of the two-pass sweep for (device, shape): zero-filled once here and left zeroed by every
    call (contract in include/dvmvs_hip.h).  Returns (tensor, bytes).

    One buffer per device and shape: calls that use it must be ordered with respect to each other, which is the case for
    the one-process-per-GPU, one-stream-per-process model of this package (a hipGraph replay runs on the stream that
    launches it).  Code that issues cost volumes of the same shape on several streams concurrently must pass its own
    workspaces through the C ABI.  Allocated outside any graph capture when the first (eager / warm-up) call happens."""
    device = torch.device(device)
    index = device.index if device.index is not None else torch.cuda.current_device()
    key = (index, B, M, H, W, D)
    entry = _workspaces.get(key)
    if entry is None:
        nbytes = _capi.lib().dvmvs_cost_volume_workspace_bytes(B, M, H, W, D)
        entry = (torch.zeros((nbytes + 3) // 4, dtype=torch.float32, device=device), nbytes)
        _workspaces[key] = entry
    return entry


def drop_sweep_workspace(device, B, M, H, W, D):
    """Forgets the cached workspace of (device, shape).  Called when a cost-volume call fails: its contract (header words zero
    between calls) may no longer hold, and a stale group count would silently corrupt every later volume of that shape."""
    device = torch.device(device)
    index = device.index if device.index is not None else torch.cuda.current_device()
    _workspaces.pop((index, B, M, H, W, D), None)


def _no_cpu(op):
    raise RuntimeError(f"dvmvs::{op} only runs as a HIP kernel on an MI355X; move the tensors to the GPU. "
                       f"There is deliberately no CPU fallback (the CPU oracle under oracle/ is for tests).")


def _dev_f32(name, *tensors):
    for t in tensors:
        if t.device.type != "cuda":
            _no_cpu(name)
        if t.dtype != torch.float32:
            raise TypeError(f"dvmvs::{name}: expected float32 tensors, got {t.dtype}")


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _ptr(t):
    return t.data_ptr()


# ----------------------------------------------------------------------------------------------------------------------
# fused plane-sweep cost volume
# ----------------------------------------------------------------------------------------------------------------------
def _check_sweep_matrices(name, Hm, kt, B, M):
    if tuple(Hm.shape) != (B, M, 9) or tuple(kt.shape) != (B, M, 3):
        raise ValueError(f"dvmvs::{name}: expected Hm [{B},{M},9] and kt [{B},{M},3] (dvmvs.pose_algebra.sweep_matrices), "
                         f"got {tuple(Hm.shape)} and {tuple(kt.shape)}")


def sweep_work_list_words(B: int, H: int, W: int, D: int) -> int:
    """32-bit words of a sweep work list for this shape (dvmvs_sweep_work_list_bytes / 4)."""
    return int(_capi.lib().dvmvs_sweep_work_list_bytes(int(B), int(H), int(W), int(D))) // 4


def sweep_work_list_host(Hm: Tensor, kt: Tensor, H: int, W: int, D: int, min_depth: float, max_depth: float, variant: int, out: Optional[Tensor] = None):
    """The tiled sweep's work list for HOST matrices ``Hm`` [B,M,9] / ``kt`` [B,M,3] (dvmvs_sweep_work_list: (tile, chunk) pairs whose
    sample boxes had to be halved are cut into plane sub-ranges that separate workgroups process in parallel), as an int32 host tensor
    (``out``: a caller-owned one, e.g. a slice of pinned staging memory).  ``variant``: the launch's (3 = wide configuration)."""
    Hm, kt = Hm.contiguous(), kt.contiguous()
    if Hm.device.type != "cpu" or Hm.dtype != torch.float32 or kt.dtype != torch.float32:
        raise ValueError("sweep_work_list_host needs the float32 HOST copies of the sweep matrices")
    B, M = Hm.shape[0], Hm.shape[1]
    words = sweep_work_list_words(B, H, W, D)
    if out is None:
        out = torch.empty(words, dtype=torch.int32)
    if out.device.type != "cpu" or out.dtype != torch.int32 or out.numel() < words or not out.is_contiguous():
        raise ValueError(f"work list buffer must be a contiguous int32 host tensor of at least {words} words")
    used = _capi.lib().dvmvs_sweep_work_list(Hm.data_ptr(), kt.data_ptr(), B, M, int(H), int(W), int(D), float(min_depth), float(max_depth),
                                             1 if variant in (3, 5) else 0, out.data_ptr(), out.numel() * 4)
    if used < 0:
        _capi.check(used, "dvmvs_sweep_work_list")
    return out


def sweep_plan_host(Hm: Tensor, kt: Tensor, H: int, W: int, D: int, min_depth: float, max_depth: float, variant: int, out: Tensor,
                    allow_mfma: bool = False) -> int:
    """Configuration choice (``variant`` 0; or 2 / 3 as given) and work list in one walk (dvmvs_sweep_plan): fills ``out`` (an int32 host
    tensor of ``sweep_work_list_words``) and returns the variant to launch with."""
    Hm, kt = Hm.contiguous(), kt.contiguous()
    if Hm.device.type != "cpu" or Hm.dtype != torch.float32 or kt.dtype != torch.float32:
        raise ValueError("sweep_plan_host needs the float32 HOST copies of the sweep matrices")
    if out.device.type != "cpu" or out.dtype != torch.int32 or not out.is_contiguous() or out.numel() < sweep_work_list_words(Hm.shape[0], H, W, D):
        raise ValueError("work list buffer must be a contiguous int32 host tensor of sweep_work_list_words entries")
    if allow_mfma and int(variant) == 0:
        # ... with variant 6 (the correlate-then-interpolate sweep) as a candidate: for callers with 32-channel channels-last measurement maps
        chosen = _capi.lib().dvmvs_sweep_plan6(Hm.data_ptr(), kt.data_ptr(), Hm.shape[0], Hm.shape[1], int(H), int(W), int(D), float(min_depth),
                                               float(max_depth), out.data_ptr(), out.numel() * 4)
    else:
        chosen = _capi.lib().dvmvs_sweep_plan(Hm.data_ptr(), kt.data_ptr(), Hm.shape[0], Hm.shape[1], int(H), int(W), int(D), float(min_depth),
                                              float(max_depth), {4: 2, 5: 3}.get(int(variant), int(variant)), out.data_ptr(), out.numel() * 4)
    if chosen < 0:
        _capi.check(chosen, "dvmvs_sweep_plan")
    return chosen


def _work_list_ptr(work_list, image1, B, H, W, D):
    if work_list is None:
        return None
    if work_list.device != image1.device or work_list.dtype != torch.int32 or not work_list.is_contiguous() or \
            work_list.numel() < sweep_work_list_words(B, H, W, D):
        raise ValueError("dvmvs::cost_volume: work_list must be a contiguous int32 tensor of dvmvs_sweep_work_list_bytes on the features' device")
    return work_list.data_ptr()


def cost_volume(image1: Tensor, image2s: Sequence[Tensor], Hm: Tensor, kt: Tensor, min_depth: float, max_depth: float, n_depth_levels: int,
                dot_product: bool, variant: int, work_list: Optional[Tensor] = None) -> Tensor:
    """``Hm`` [B,M,9] = K R K^-1 and ``kt`` [B,M,3] = K t per (batch item, measurement frame): dvmvs.pose_algebra.  ``work_list``: the
    device copy of ``sweep_work_list_host``'s result for these matrices (optional; the tiled sweep then cuts long workgroups).
    Differentiable in the feature maps (dot-product mode)."""
    if work_list is None:      # (the registered op takes a tensor: an empty one = no list)
        work_list = torch.empty(0, dtype=torch.int32, device=image1.device)
    return _cost_volume_op(image1, image2s, Hm, kt, min_depth, max_depth, n_depth_levels, dot_product, variant, work_list)


@torch.library.custom_op("dvmvs::cost_volume", mutates_args=(), device_types="cuda")
def _cost_volume_op(image1: Tensor, image2s: Sequence[Tensor], Hm: Tensor, kt: Tensor,
                    min_depth: float, max_depth: float, n_depth_levels: int, dot_product: bool, variant: int, work_list: Tensor) -> Tensor:
    _dev_f32("cost_volume", image1, Hm, kt, *image2s)
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
    Hm, kt = Hm.contiguous(), kt.contiguous()
    out = torch.empty((B, n_depth_levels, H, W), dtype=torch.float32, device=image1.device)
    lib = _capi.lib()
    workspace, ws_bytes = sweep_workspace(image1.device, B, M, H, W, n_depth_levels) if COST_VOLUME_TWO_PASS else (None, 0)
    items = _work_list_ptr(work_list if work_list.numel() else None, image1, B, H, W, n_depth_levels)
    with torch.cuda.device(image1.device):
        rc = lib.dvmvs_cost_volume_planned_fwd(
            _ptr(image1), _capi.pointer_array([_ptr(t) for t in image2s]), _ptr(Hm), _ptr(kt), _ptr(out),
            B, M, C, H, W, n_depth_levels, float(min_depth), float(max_depth), int(bool(dot_product)), int(variant),
            _capi.LAYOUT_NHWC if nhwc else _capi.LAYOUT_NCHW, _ptr(workspace) if workspace is not None else None, ws_bytes, items, _stream(image1))
    if rc != 0 and workspace is not None:
        drop_sweep_workspace(image1.device, B, M, H, W, n_depth_levels)
    _capi.check(rc, "dvmvs_cost_volume_planned_fwd")
    return out


@_cost_volume_op.register_fake
def _(image1, image2s, Hm, kt, min_depth, max_depth, n_depth_levels, dot_product, variant, work_list):
    B, C, H, W = image1.shape
    return image1.new_empty((B, n_depth_levels, H, W))


@_cost_volume_op.register_kernel("cpu")
def _(image1, image2s, Hm, kt, min_depth, max_depth, n_depth_levels, dot_product, variant, work_list):
    _no_cpu("cost_volume")


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
    with torch.cuda.device(image1.device):
        rc = _capi.lib().dvmvs_cost_volume_bwd(
            _ptr(grad), _ptr(image1c), _capi.pointer_array([_ptr(t) for t in image2c]), _ptr(Hm.contiguous()), _ptr(kt.contiguous()),
            _ptr(g1), _capi.pointer_array([_ptr(t) for t in g2] if need2 else [None] * M),
            B, M, C, H, W, D, float(min_depth), float(max_depth), _stream(image1))
    _capi.check(rc, "dvmvs_cost_volume_bwd")
    return g1, (g2 if need2 else [None] * M), None, None, None, None, None, None, None, None


torch.library.register_autograd("dvmvs::cost_volume", _cost_volume_backward, setup_context=_cost_volume_setup)


@torch.library.custom_op("dvmvs::sweep_matrices", mutates_args=(), device_types="cuda")
def sweep_matrices(pose1: Tensor, pose2s: Sequence[Tensor], K: Tensor) -> Tuple[Tensor, Tensor]:
    """"exact" pose algebra: (Hm [B,M,9], kt [B,M,3]) in fp64 on the device, rounded once (dvmvs_sweep_matrices)."""
    _dev_f32("sweep_matrices", pose1, K, *pose2s)
    B, M = pose1.shape[0], len(pose2s)
    if M == 0 or tuple(pose1.shape) != (B, 4, 4) or tuple(K.shape) != (B, 3, 3) or any(tuple(p.shape) != (B, 4, 4) for p in pose2s):
        raise ValueError("dvmvs::sweep_matrices: expected pose1 [B,4,4], M >= 1 measurement poses [B,4,4] and K [B,3,3]")
    pose1, K = pose1.contiguous(), K.contiguous()
    pose2s = [p.contiguous() for p in pose2s]
    Hm = torch.empty((B, M, 9), dtype=torch.float32, device=pose1.device)
    kt = torch.empty((B, M, 3), dtype=torch.float32, device=pose1.device)
    with torch.cuda.device(pose1.device):
        rc = _capi.lib().dvmvs_sweep_matrices(_ptr(pose1), _capi.pointer_array([_ptr(p) for p in pose2s]), _ptr(K), _ptr(Hm), _ptr(kt),
                                              B, M, _stream(pose1))
    _capi.check(rc, "dvmvs_sweep_matrices")
    return Hm, kt


@sweep_matrices.register_fake
def _(pose1, pose2s, K):
    B, M = pose1.shape[0], len(pose2s)
    return pose1.new_empty((B, M, 9)), pose1.new_empty((B, M, 3))


@sweep_matrices.register_kernel("cpu")
def _(pose1, pose2s, K):
    _no_cpu("sweep_matrices")


# ----------------------------------------------------------------------------------------------------------------------
# hidden-state warp
# ----------------------------------------------------------------------------------------------------------------------
@torch.library.custom_op("dvmvs::hidden_warp", mutates_args=(), device_types="cuda")
def hidden_warp(image_src: Tensor, depth_dst: Tensor, src_trans_dst: Tensor, camera_matrix: Tensor,
                zero_invalid: bool) -> Tensor:
    _dev_f32("hidden_warp", image_src, depth_dst, src_trans_dst, camera_matrix)
    B, C, H, W = image_src.shape
    image_src, depth_dst = image_src.contiguous(), depth_dst.contiguous()
    src_trans_dst, camera_matrix = src_trans_dst.contiguous(), camera_matrix.contiguous()
    out = torch.empty_like(image_src)
    with torch.cuda.device(image_src.device):
        rc = _capi.lib().dvmvs_hidden_warp_fwd(_ptr(image_src), _ptr(depth_dst), _ptr(src_trans_dst), _ptr(camera_matrix),
                                               _ptr(out), B, C, H, W, int(bool(zero_invalid)), _stream(image_src))
    _capi.check(rc, "dvmvs_hidden_warp_fwd")
    return out


@hidden_warp.register_fake
def _(image_src, depth_dst, src_trans_dst, camera_matrix, zero_invalid):
    return torch.empty_like(image_src)


@hidden_warp.register_kernel("cpu")
def _(image_src, depth_dst, src_trans_dst, camera_matrix, zero_invalid):
    _no_cpu("hidden_warp")


def _hidden_warp_setup(ctx, inputs, output):
    image_src, depth_dst, src_trans_dst, camera_matrix, _ = inputs
    ctx.shape = tuple(image_src.shape)
    ctx.save_for_backward(depth_dst, src_trans_dst, camera_matrix)


def _hidden_warp_backward(ctx, grad):
    depth_dst, src_trans_dst, camera_matrix = ctx.saved_tensors
    B, C, H, W = ctx.shape
    grad = grad.contiguous()
    gsrc = torch.zeros_like(grad)
    with torch.cuda.device(grad.device):
        # the validity mask is NOT applied to the gradient, as in the reference (convlstm.py:41 edits .data)
        rc = _capi.lib().dvmvs_hidden_warp_bwd(_ptr(grad), _ptr(depth_dst.contiguous()), _ptr(src_trans_dst.contiguous()),
                                               _ptr(camera_matrix.contiguous()), _ptr(gsrc), B, C, H, W, _stream(grad))
    _capi.check(rc, "dvmvs_hidden_warp_bwd")
    return gsrc, None, None, None, None


torch.library.register_autograd("dvmvs::hidden_warp", _hidden_warp_backward, setup_context=_hidden_warp_setup)


# ----------------------------------------------------------------------------------------------------------------------
# inverse(a) @ c for 4x4 poses, fp64 on the device ("exact" pose algebra; the default path is dvmvs.pose_algebra's host fp32)
# ----------------------------------------------------------------------------------------------------------------------
@torch.library.custom_op("dvmvs::relative_pose", mutates_args=(), device_types="cuda")
def relative_pose(a: Tensor, c: Tensor) -> Tensor:
    _dev_f32("relative_pose", a, c)
    if a.shape != c.shape or a.shape[-2:] != (4, 4) or a.dim() != 3:
        raise ValueError(f"dvmvs::relative_pose: expected two [B,4,4] tensors, got {tuple(a.shape)} and {tuple(c.shape)}")
    a, c = a.contiguous(), c.contiguous()
    out = torch.empty_like(a)
    with torch.cuda.device(a.device):
        rc = _capi.lib().dvmvs_relative_pose(_ptr(a), _ptr(c), _ptr(out), a.shape[0], _stream(a))
    _capi.check(rc, "dvmvs_relative_pose")
    return out


@relative_pose.register_fake
def _(a, c):
    return torch.empty_like(a)


@relative_pose.register_kernel("cpu")
def _(a, c):
    _no_cpu("relative_pose")


# ----------------------------------------------------------------------------------------------------------------------
# ConvLSTM gate fusion
# ----------------------------------------------------------------------------------------------------------------------
@torch.library.custom_op("dvmvs::lstm_gates", mutates_args=(), device_types="cuda")
def lstm_gates(combined_conv: Tensor, c_cur: Tensor) -> Tuple[Tensor, Tensor]:
    _dev_f32("lstm_gates", combined_conv, c_cur)
    B, hidden, H, W = c_cur.shape
    if combined_conv.shape != (B, 4 * hidden, H, W):
        raise ValueError(f"dvmvs::lstm_gates: conv output {tuple(combined_conv.shape)} does not match state {tuple(c_cur.shape)}")
    combined_conv, c_cur = combined_conv.contiguous(), c_cur.contiguous()
    h_next, c_next = torch.empty_like(c_cur), torch.empty_like(c_cur)
    with torch.cuda.device(c_cur.device):
        rc = _capi.lib().dvmvs_lstm_gates_fwd(_ptr(combined_conv), _ptr(c_cur), _ptr(h_next), _ptr(c_next), B, hidden, H, W,
                                              _stream(c_cur))
    _capi.check(rc, "dvmvs_lstm_gates_fwd")
    return h_next, c_next


@lstm_gates.register_fake
def _(combined_conv, c_cur):
    return torch.empty_like(c_cur), torch.empty_like(c_cur)


@lstm_gates.register_kernel("cpu")
def _(combined_conv, c_cur):
    _no_cpu("lstm_gates")


def _lstm_gates_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)


def _lstm_gates_backward(ctx, grad_h, grad_c):
    combined_conv, c_cur = ctx.saved_tensors
    B, hidden, H, W = c_cur.shape
    cc, cs = combined_conv.contiguous(), c_cur.contiguous()
    gh = grad_h.contiguous() if grad_h is not None else None
    gc = grad_c.contiguous() if grad_c is not None else None
    grad_cc, grad_cs = torch.empty_like(cc), torch.empty_like(cs)
    with torch.cuda.device(cs.device):
        rc = _capi.lib().dvmvs_lstm_gates_bwd(_ptr(gh) if gh is not None else None, _ptr(gc) if gc is not None else None,
                                              _ptr(cc), _ptr(cs), _ptr(grad_cc), _ptr(grad_cs), B, hidden, H, W, _stream(cs))
    _capi.check(rc, "dvmvs_lstm_gates_bwd")
    return grad_cc, grad_cs


torch.library.register_autograd("dvmvs::lstm_gates", _lstm_gates_backward, setup_context=_lstm_gates_setup)


# ----------------------------------------------------------------------------------------------------------------------
# depth re-projection (forward splat)
# ----------------------------------------------------------------------------------------------------------------------
def _reproject(name, transformation, previous_depth, full_K, half_K, factor):
    _dev_f32(name, transformation, previous_depth, full_K, half_K)
    B, one, Hf, Wf = previous_depth.shape
    if one != 1:
        raise ValueError(f"dvmvs::{name}: previous depth must be [B,1,H,W], got {tuple(previous_depth.shape)}")
    if tuple(transformation.shape) != (B, 4, 4):
        raise ValueError(f"dvmvs::{name}: transformation must be [{B},4,4] (inverse(reference_pose) @ measurement_pose), "
                         f"got {tuple(transformation.shape)}")
    args = [t.contiguous() for t in (transformation, previous_depth, full_K, half_K)]
    out = torch.empty((B, 1, Hf // 2, Wf // 2), dtype=torch.float32, device=previous_depth.device)
    low = None
    if factor > 0:
        low = torch.empty((B, 1, (Hf // 2) // factor, (Wf // 2) // factor), dtype=torch.float32, device=previous_depth.device)
    with torch.cuda.device(previous_depth.device):
        rc = _capi.lib().dvmvs_depth_reproject_fwd(*[_ptr(t) for t in args], _ptr(out), _ptr(low) if low is not None else None,
                                                   int(factor), B, Hf, Wf, _stream(previous_depth))
    _capi.check(rc, "dvmvs_depth_reproject_fwd")
    return out, low


@torch.library.custom_op("dvmvs::depth_reproject", mutates_args=(), device_types="cuda")
def depth_reproject(transformation: Tensor, previous_depth: Tensor, full_K: Tensor, half_K: Tensor) -> Tensor:
    """``transformation`` [B,4,4] = inverse(reference_pose) @ measurement_pose (dvmvs.pose_algebra.relative_pose)."""
    return _reproject("depth_reproject", transformation, previous_depth, full_K, half_K, 0)[0]


@depth_reproject.register_fake
def _(transformation, previous_depth, full_K, half_K):
    B, _, Hf, Wf = previous_depth.shape
    return previous_depth.new_empty((B, 1, Hf // 2, Wf // 2))


@depth_reproject.register_kernel("cpu")
def _(transformation, previous_depth, full_K, half_K):
    _no_cpu("depth_reproject")


@torch.library.custom_op("dvmvs::depth_reproject_lowres", mutates_args=(), device_types="cuda")
def depth_reproject_lowres(transformation: Tensor, previous_depth: Tensor, full_K: Tensor, half_K: Tensor,
                           factor: int) -> Tuple[Tensor, Tensor]:
    """Splat plus the nearest /factor decimation the fusionnet call site applies next (one C-ABI call)."""
    if factor <= 0:
        raise ValueError("dvmvs::depth_reproject_lowres: factor must be positive")
    out, low = _reproject("depth_reproject_lowres", transformation, previous_depth, full_K, half_K, factor)
    return out, low


@depth_reproject_lowres.register_fake
def _(transformation, previous_depth, full_K, half_K, factor):
    B, _, Hf, Wf = previous_depth.shape
    return (previous_depth.new_empty((B, 1, Hf // 2, Wf // 2)),
            previous_depth.new_empty((B, 1, (Hf // 2) // factor, (Wf // 2) // factor)))


@depth_reproject_lowres.register_kernel("cpu")
def _(transformation, previous_depth, full_K, half_K, factor):
    _no_cpu("depth_reproject_lowres")


# ----------------------------------------------------------------------------------------------------------------------
# frame-path epilogues (inference only: no autograd formulas are registered)
# ----------------------------------------------------------------------------------------------------------------------
ACTIVATIONS = {"none": 0, "relu": 1, "sigmoid": 2}


RESIDUAL_NONE, RESIDUAL_SAME, RESIDUAL_NEAREST_UP2 = 0, 1, 2


@torch.library.custom_op("dvmvs::bias_act_", mutates_args=("x",), device_types="cuda")
def bias_act_(x: Tensor, bias: Tensor, activation: int, residual: Tensor, residual_mode: int) -> None:
    """In place: x[b,c] = act(x[b,c] + bias[c]) (+ residual) for a contiguous NCHW tensor.  ``bias`` / ``residual`` may be
    empty (numel 0); residual_mode 1: same shape, 2: half resolution, nearest-up-sampled on the fly."""
    _dev_f32("bias_act_", x)
    if not x.is_contiguous() or x.dim() != 4:
        raise ValueError("dvmvs::bias_act_: expected a contiguous NCHW tensor")
    B, C, H, W = x.shape
    if bias.numel() not in (0, C):
        raise ValueError(f"dvmvs::bias_act_: bias has {bias.numel()} entries for {C} channels")
    res_ptr = None
    if residual_mode != RESIDUAL_NONE:
        want = (B, C, H, W) if residual_mode == RESIDUAL_SAME else (B, C, H // 2, W // 2)
        if tuple(residual.shape) != want:
            raise ValueError(f"dvmvs::bias_act_: residual {tuple(residual.shape)} does not match {want}")
        residual = residual.contiguous()
        res_ptr = _ptr(residual)
    with torch.cuda.device(x.device):
        rc = _capi.lib().dvmvs_bias_act_inplace(_ptr(x), _ptr(bias.contiguous()) if bias.numel() else None, res_ptr, int(residual_mode),
                                                B, C, H, W, int(activation), _stream(x))
    _capi.check(rc, "dvmvs_bias_act_inplace")


@bias_act_.register_kernel("cpu")
def _(x, bias, activation, residual, residual_mode):
    _no_cpu("bias_act_")


@torch.library.custom_op("dvmvs::upsample2x", mutates_args=(), device_types="cuda")
def upsample2x(x: Tensor) -> Tensor:
    _dev_f32("upsample2x", x)
    x = x.contiguous()
    B, C, H, W = x.shape
    out = torch.empty((B, C, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = _capi.lib().dvmvs_upsample2x_fwd(_ptr(x), _ptr(out), 0, None, 0, B, C, H, W, _stream(x))
    _capi.check(rc, "dvmvs_upsample2x_fwd")
    return out


@upsample2x.register_fake
def _(x):
    B, C, H, W = x.shape
    return x.new_empty((B, C, 2 * H, 2 * W))


@upsample2x.register_kernel("cpu")
def _(x):
    _no_cpu("upsample2x")


@torch.library.custom_op("dvmvs::upsample2x_bwd", mutates_args=(), device_types="cuda")
def upsample2x_bwd(grad_out: Tensor) -> Tensor:
    """Adjoint of ``upsample2x`` as a gather (no atomics: bit-reproducible), dvmvs_upsample2x_bwd."""
    _dev_f32("upsample2x_bwd", grad_out)
    grad_out = grad_out.contiguous()
    B, C, OH, OW = grad_out.shape
    grad_in = torch.empty((B, C, OH // 2, OW // 2), dtype=torch.float32, device=grad_out.device)
    with torch.cuda.device(grad_out.device):
        rc = _capi.lib().dvmvs_upsample2x_bwd(_ptr(grad_out), _ptr(grad_in), B, C, OH // 2, OW // 2, _stream(grad_out))
    _capi.check(rc, "dvmvs_upsample2x_bwd")
    return grad_in


@upsample2x_bwd.register_fake
def _(grad_out):
    B, C, OH, OW = grad_out.shape
    return grad_out.new_empty((B, C, OH // 2, OW // 2))


torch.library.register_autograd("dvmvs::upsample2x", lambda ctx, grad: upsample2x_bwd(grad), setup_context=lambda ctx, inputs, output: None)


@torch.library.custom_op("dvmvs::depthwise_conv_train", mutates_args=(), device_types="cuda")
def depthwise_conv_train(x: Tensor, weight: Tensor, stride: int) -> Tensor:
    """Depthwise k x k convolution (weight [C,1,k,k], padding k//2, no bias) with gradients: the training-time form of
    ``depthwise_conv`` (MIOpen runs these MnasNet layers, forward and backward, through its naive reference kernels)."""
    _dev_f32("depthwise_conv_train", x, weight)
    x, weight = x.contiguous(), weight.contiguous()
    B, C, H, W = x.shape
    k = weight.shape[-1]
    if tuple(weight.shape) != (C, 1, k, k):
        raise ValueError(f"dvmvs::depthwise_conv_train: weight {tuple(weight.shape)} is not depthwise for {C} channels")
    pad = k // 2
    out = torch.empty((B, C, (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = _capi.lib().dvmvs_depthwise_conv_fwd(_ptr(x), _ptr(weight), None, None, 0, _ptr(out), B, C, H, W, k, int(stride), 0, _stream(x))
    _capi.check(rc, "dvmvs_depthwise_conv_fwd")
    return out


@depthwise_conv_train.register_fake
def _(x, weight, stride):
    B, C, H, W = x.shape
    k = weight.shape[-1]
    pad = k // 2
    return x.new_empty((B, C, (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1))


@torch.library.custom_op("dvmvs::depthwise_conv_bwd", mutates_args=(), device_types="cuda")
def depthwise_conv_bwd(grad_out: Tensor, x: Tensor, weight: Tensor, stride: int, need_input: bool, need_weight: bool) -> Tuple[Tensor, Tensor]:
    """(grad_x, grad_weight) of ``depthwise_conv_train`` (gathers / a fixed-order reduction: no atomics); an unneeded one is empty."""
    _dev_f32("depthwise_conv_bwd", grad_out, x, weight)
    grad_out, x, weight = grad_out.contiguous(), x.contiguous(), weight.contiguous()
    B, C, H, W = x.shape
    k = weight.shape[-1]
    gx = torch.empty_like(x) if need_input else x.new_empty(0)
    gw = torch.empty_like(weight) if need_weight else x.new_empty(0)
    lib = _capi.lib()
    scratch = lib.dvmvs_depthwise_conv_bwd_workspace_bytes(B, C, H, W, k, int(stride)) if need_weight else 0
    workspace = torch.empty(scratch // 4, dtype=torch.float32, device=x.device) if scratch else None
    with torch.cuda.device(x.device):
        rc = lib.dvmvs_depthwise_conv_bwd(_ptr(grad_out), _ptr(x), _ptr(weight), _ptr(gx) if need_input else None,
                                          _ptr(gw) if need_weight else None, _ptr(workspace) if workspace is not None else None,
                                          B, C, H, W, k, int(stride), _stream(x))
    _capi.check(rc, "dvmvs_depthwise_conv_bwd")
    return gx, gw


@depthwise_conv_bwd.register_fake
def _(grad_out, x, weight, stride, need_input, need_weight):
    return (torch.empty_like(x) if need_input else x.new_empty(0)), (torch.empty_like(weight) if need_weight else x.new_empty(0))


def _depthwise_train_setup(ctx, inputs, output):
    x, weight, stride = inputs
    ctx.stride = stride
    ctx.save_for_backward(x, weight)


def _depthwise_train_backward(ctx, grad):
    x, weight = ctx.saved_tensors
    need_input, need_weight = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    gx, gw = depthwise_conv_bwd(grad, x, weight, ctx.stride, need_input, need_weight)
    return (gx if need_input else None), (gw if need_weight else None), None


torch.library.register_autograd("dvmvs::depthwise_conv_train", _depthwise_train_backward, setup_context=_depthwise_train_setup)


@torch.library.custom_op("dvmvs::depthwise_conv", mutates_args=(), device_types="cuda")
def depthwise_conv(x: Tensor, weight: Tensor, bias: Tensor, stride: int, activation: int, pre_bias: Tensor, pre_relu: bool) -> Tensor:
    """Depthwise k x k convolution (weight [C,1,k,k], padding k//2) + bias (numel 0 = none) + activation, one HIP launch.  With
    ``pre_relu`` the input is the raw output of the preceding 1x1 convolution and relu(x + pre_bias[c]) (numel 0 = no bias) is applied
    to it on the fly."""
    _dev_f32("depthwise_conv", x, weight)
    x, weight = x.contiguous(), weight.contiguous()
    B, C, H, W = x.shape
    k = weight.shape[-1]
    if tuple(weight.shape) != (C, 1, k, k):
        raise ValueError(f"dvmvs::depthwise_conv: weight {tuple(weight.shape)} is not depthwise for {C} channels")
    pad = k // 2
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    out = torch.empty((B, C, OH, OW), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        if pre_bias.numel() not in (0, C):
            raise ValueError(f"dvmvs::depthwise_conv: pre_bias has {pre_bias.numel()} entries for {C} channels")
        rc = _capi.lib().dvmvs_depthwise_conv_fwd(_ptr(x), _ptr(weight), _ptr(bias.contiguous()) if bias.numel() else None,
                                                  _ptr(pre_bias.contiguous()) if pre_bias.numel() else None, int(bool(pre_relu)), _ptr(out),
                                                  B, C, H, W, k, int(stride), int(activation), _stream(x))
    _capi.check(rc, "dvmvs_depthwise_conv_fwd")
    return out


@depthwise_conv.register_fake
def _(x, weight, bias, stride, activation, pre_bias, pre_relu):
    B, C, H, W = x.shape
    k = weight.shape[-1]
    pad = k // 2
    return x.new_empty((B, C, (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1))


@depthwise_conv.register_kernel("cpu")
def _(x, weight, bias, stride, activation, pre_bias, pre_relu):
    _no_cpu("depthwise_conv")


# ----------------------------------------------------------------------------------------------------------------------
# destination-passing forms for the frame engine (inference, no autograd, hipGraph-capturable): the producer writes straight
# into a channel slice of a concatenation buffer or into a state buffer, so that torch.cat / copy_ launches disappear from
# the frame.  Plain functions over the C ABI, not torch.library ops: nothing here allocates or needs shape inference.
# ----------------------------------------------------------------------------------------------------------------------
ACTIVATION_SIGMOID_TO_DEPTH = 3


def _slice_batch_stride(name, dst, B, C, H, W):
    """``dst`` must be [B,C,H,W] with dense planes and channels (a channel slice of a contiguous NCHW buffer); returns its batch
    stride in elements."""
    if dst.device.type != "cuda" or dst.dtype != torch.float32:
        raise TypeError(f"dvmvs::{name}: destination must be a float32 HIP tensor")
    if tuple(dst.shape) != (B, C, H, W) or dst.stride(3) != 1 or dst.stride(2) != W or dst.stride(1) != H * W:
        raise ValueError(f"dvmvs::{name}: destination {tuple(dst.shape)} / strides {dst.stride()} is not a channel slice of a "
                         f"contiguous NCHW buffer for [{B},{C},{H},{W}]")
    return dst.stride(0) if B > 1 else C * H * W


def bias_act_into(x: Tensor, dst: Tensor, bias, activation: int, residual=None, residual_mode: int = RESIDUAL_NONE, p0: float = 0.0,
                  p1: float = 0.0) -> Tensor:
    """dst = act(x + bias[c]) (+ residual); ``x`` a dense convolution output, ``dst`` x itself or a channel slice (see above)."""
    _dev_f32("bias_act_into", x)
    if not x.is_contiguous() or x.dim() != 4:
        raise ValueError("dvmvs::bias_act_into: expected a contiguous NCHW source")
    B, C, H, W = x.shape
    stride = _slice_batch_stride("bias_act_into", dst, B, C, H, W)
    if bias is not None and bias.numel() not in (0, C):
        raise ValueError(f"dvmvs::bias_act_into: bias has {bias.numel()} entries for {C} channels")
    res_ptr = None
    if residual_mode != RESIDUAL_NONE:
        want = (B, C, H, W) if residual_mode == RESIDUAL_SAME else (B, C, H // 2, W // 2)
        if tuple(residual.shape) != want or not residual.is_contiguous():
            raise ValueError(f"dvmvs::bias_act_into: residual {tuple(residual.shape)} does not match {want} (contiguous)")
        res_ptr = _ptr(residual)
    with torch.cuda.device(x.device):
        rc = _capi.lib().dvmvs_bias_act_fwd(_ptr(x), _ptr(dst), stride, _ptr(bias) if bias is not None and bias.numel() else None, res_ptr,
                                            int(residual_mode), B, C, H, W, int(activation), float(p0), float(p1), _stream(x))
    _capi.check(rc, "dvmvs_bias_act_fwd")
    return dst


EUNSUPPORTED = -2     # include/dvmvs_hip.h


def conv_bias_act_into(x: Tensor, weight: Tensor, bias: Tensor, dst, stride: int, padding: int, activation: int):
    """conv2d(x, weight, padding, stride) + bias [+ ReLU] as ONE MIOpen fusion plan (dvmvs_conv_bias_act_fwd), written into ``dst``
    (a dense tensor or a channel slice of a concatenation buffer; None: a new tensor).  Returns the output, or None when MIOpen has
    no fused plan for the problem (the caller then runs convolution + dvmvs_bias_act_fwd)."""
    _dev_f32("conv_bias_act_into", x, weight, bias)
    if activation not in (ACTIVATIONS["none"], ACTIVATIONS["relu"]):
        raise ValueError("dvmvs::conv_bias_act_into: activation must be none or relu")
    x, weight = x.contiguous(), weight.contiguous()
    B, Cin, H, W = x.shape
    Cout, Cin_w, K, K2 = weight.shape
    if Cin_w != Cin or K != K2 or bias.numel() != Cout:
        raise ValueError(f"dvmvs::conv_bias_act_into: weight {tuple(weight.shape)} / bias {bias.numel()} do not fit input {tuple(x.shape)}")
    Ho, Wo = (H + 2 * padding - K) // stride + 1, (W + 2 * padding - K) // stride + 1
    if dst is None:
        dst = torch.empty(B, Cout, Ho, Wo, device=x.device, dtype=torch.float32)
    batch_stride = _slice_batch_stride("conv_bias_act_into", dst, B, Cout, Ho, Wo)
    with torch.cuda.device(x.device):
        rc = _capi.lib().dvmvs_conv_bias_act_fwd(_ptr(x), _ptr(weight), _ptr(bias), _ptr(dst), batch_stride, B, Cin, H, W, Cout, K,
                                                 int(stride), int(padding), int(activation), _stream(x))
    if rc == EUNSUPPORTED:
        return None
    _capi.check(rc, "dvmvs_conv_bias_act_fwd")
    return dst


def upsample2x_into(x: Tensor, dst: Tensor, pre_bias=None, pre_activation: int = 0) -> Tensor:
    """x2 bilinear (align_corners) up-sampling of ``x`` into ``dst``; with ``pre_activation`` (ACTIVATIONS) ``x`` is a raw convolution
    output and act(x + pre_bias[c]) is applied to the taps on the fly."""
    _dev_f32("upsample2x_into", x)
    x = x.contiguous()
    B, C, H, W = x.shape
    stride = _slice_batch_stride("upsample2x_into", dst, B, C, 2 * H, 2 * W)
    if pre_bias is not None and pre_bias.numel() not in (0, C):
        raise ValueError(f"dvmvs::upsample2x_into: pre_bias has {pre_bias.numel()} entries for {C} channels")
    with torch.cuda.device(x.device):
        rc = _capi.lib().dvmvs_upsample2x_fwd(_ptr(x), _ptr(dst), stride, _ptr(pre_bias) if pre_bias is not None and pre_bias.numel() else None,
                                              int(pre_activation), B, C, H, W, _stream(x))
    _capi.check(rc, "dvmvs_upsample2x_fwd")
    return dst


def upsample2x_pair_into(x1: Tensor, dst1: Tensor, x2: Tensor, dst2: Tensor, pre_bias2=None, pre_activation2: int = 0) -> None:
    """``upsample2x_into(x1, dst1)`` and ``upsample2x_into(x2, dst2, pre_bias2, pre_activation2)`` for two maps of the same size in ONE launch
    (dvmvs_upsample2x_pair_fwd: a decoder level's feature map and its depth head); the same values bit for bit."""
    _dev_f32("upsample2x_pair_into", x1, x2)
    x1, x2 = x1.contiguous(), x2.contiguous()
    B, C1, H, W = x1.shape
    C2 = x2.shape[1]
    if tuple(x2.shape) != (B, C2, H, W):
        raise ValueError(f"dvmvs::upsample2x_pair_into: the two maps must have the same batch and size, got {tuple(x1.shape)} and {tuple(x2.shape)}")
    stride1 = _slice_batch_stride("upsample2x_pair_into", dst1, B, C1, 2 * H, 2 * W)
    stride2 = _slice_batch_stride("upsample2x_pair_into", dst2, B, C2, 2 * H, 2 * W)
    if pre_bias2 is not None and pre_bias2.numel() not in (0, C2):
        raise ValueError(f"dvmvs::upsample2x_pair_into: pre_bias2 has {pre_bias2.numel()} entries for {C2} channels")
    with torch.cuda.device(x1.device):
        rc = _capi.lib().dvmvs_upsample2x_pair_fwd(_ptr(x1), _ptr(dst1), stride1, C1, _ptr(x2), _ptr(dst2), stride2,
                                                   _ptr(pre_bias2) if pre_bias2 is not None and pre_bias2.numel() else None, int(pre_activation2), C2, B, H, W,
                                                   _stream(x1))
    _capi.check(rc, "dvmvs_upsample2x_pair_fwd")


def lstm_gates_into(combined_conv: Tensor, c_state: Tensor, h_state: Tensor) -> None:
    """State update in place: c_state <- c', h_state <- h' (the kernel reads a row of c completely before it writes it)."""
    _dev_f32("lstm_gates_into", combined_conv, c_state, h_state)
    B, hidden, H, W = c_state.shape
    if tuple(combined_conv.shape) != (B, 4 * hidden, H, W) or tuple(h_state.shape) != tuple(c_state.shape):
        raise ValueError("dvmvs::lstm_gates_into: shapes do not match")
    if not (combined_conv.is_contiguous() and c_state.is_contiguous() and h_state.is_contiguous()):
        raise ValueError("dvmvs::lstm_gates_into: expected contiguous tensors")
    with torch.cuda.device(c_state.device):
        rc = _capi.lib().dvmvs_lstm_gates_fwd(_ptr(combined_conv), _ptr(c_state), _ptr(h_state), _ptr(c_state), B, hidden, H, W, _stream(c_state))
    _capi.check(rc, "dvmvs_lstm_gates_fwd")


# ---- 3x3 convolutions on the bottleneck maps (csrc/bottleneck_conv.hip): weight-streaming fp32 MFMA GEMM, deterministic split-K ----
def bottleneck_conv_splits(B: int, C_out: int, C_in: int, H_in: int, W_in: int, stride: int) -> int:
    """Number of K-splits (partial sums) dvmvs_bottleneck_conv_fwd produces for this problem; 0 when the kernel does not take it
    (other map sizes, C_in not a multiple of 16): the caller stays on MIOpen."""
    n = _capi.lib().dvmvs_bottleneck_conv_splits(int(B), int(C_out), int(C_in), int(H_in), int(W_in), int(stride))
    return n if n > 0 else 0


def bottleneck_conv_pack(weight: Tensor) -> Tensor:
    """[C_out, C_in, 3, 3] convolution weights re-packed once into the MFMA A-operand order the kernel streams."""
    _dev_f32("bottleneck_conv_pack", weight)
    C_out, C_in, kh, kw = weight.shape
    nbytes = _capi.lib().dvmvs_bottleneck_conv_packed_bytes(C_out, C_in) if (kh, kw) == (3, 3) else 0
    if nbytes == 0:
        raise ValueError(f"dvmvs::bottleneck_conv_pack: need a 3x3 kernel and C_in % 16 == 0, got {tuple(weight.shape)}")
    packed = torch.empty(nbytes // 4, dtype=torch.float32, device=weight.device)
    with torch.cuda.device(weight.device):
        rc = _capi.lib().dvmvs_bottleneck_conv_pack(_ptr(weight.contiguous()), _ptr(packed), C_out, C_in, _stream(weight))
    _capi.check(rc, "dvmvs_bottleneck_conv_pack")
    return packed


def bottleneck_conv_into(x: Tensor, packed: Tensor, C_out: int, stride: int, partials: Tensor, upsample: bool = False) -> int:
    """3x3, padding 1 convolution of ``x`` [B,C_in,H,W] with ``bottleneck_conv_pack``-ed weights as K-split partial sums into
    ``partials`` (at least splits * B * C_out * H_out * W_out floats, laid out [split][B][C_out][H_out*W_out]).  Returns the number of
    splits; the consumer adds them in ascending order (``partial_sums_bias_act_into`` / ``lstm_gates_partials_into``).
    ``upsample``: the layer convolves the 2x bilinear up-sampling (align_corners=True, ``upsample2x``'s values bit for bit) of ``x``
    [B,C_in,H/2,W/2], interpolated while the input is staged (dvmvs_bottleneck_conv_up2x_fwd: the 16x20 map, stride 1)."""
    _dev_f32("bottleneck_conv_into", x, packed, partials)
    B, C_in, H, W = x.shape
    if upsample:
        H, W = 2 * H, 2 * W
    splits = bottleneck_conv_splits(B, C_out, C_in, H, W, stride) if not upsample or (H, W, stride) == (16, 20, 1) else 0
    if splits == 0:
        raise ValueError(f"dvmvs::bottleneck_conv_into: problem {tuple(x.shape)} -> {C_out} (stride {stride}{', up-sampled' if upsample else ''}) "
                         f"is not one of the bottleneck shapes")
    if not x.is_contiguous() or partials.numel() < splits * B * C_out * (H // stride) * (W // stride) or not partials.is_contiguous():
        raise ValueError("dvmvs::bottleneck_conv_into: expected a contiguous input and a partial-sum buffer of splits * B * C_out * H_out * W_out floats")
    with torch.cuda.device(x.device):
        if upsample:
            rc = _capi.lib().dvmvs_bottleneck_conv_up2x_fwd(_ptr(x), _ptr(packed), _ptr(partials), B, C_in, H, W, int(C_out), _stream(x))
        else:
            rc = _capi.lib().dvmvs_bottleneck_conv_fwd(_ptr(x), _ptr(packed), _ptr(partials), B, C_in, H, W, int(C_out), int(stride), _stream(x))
    _capi.check(rc, "dvmvs_bottleneck_conv_fwd")
    return splits


def partial_sums_bias_act_into(partials: Tensor, n_partials: int, dst: Tensor, bias, activation: int, shape) -> Tensor:
    """dst = act(sum of the partial sums + bias[c]); ``dst`` a dense [B,C,H,W] tensor or a channel slice of a concatenation buffer."""
    _dev_f32("partial_sums_bias_act_into", partials, dst)
    B, C, H, W = shape
    stride = _slice_batch_stride("partial_sums_bias_act_into", dst, B, C, H, W)
    with torch.cuda.device(dst.device):
        rc = _capi.lib().dvmvs_partial_sums_bias_act_fwd(_ptr(partials), int(n_partials), _ptr(dst), stride,
                                                         _ptr(bias) if bias is not None and bias.numel() else None, B, C, H * W, int(activation),
                                                         _stream(dst))
    _capi.check(rc, "dvmvs_partial_sums_bias_act_fwd")
    return dst


# ---- dense 3x3 / 5x5 convolutions of the larger maps (csrc/direct_conv.hip): direct fp32 MFMA convolution, bias + ReLU fused ----
def direct_conv_tile(B: int, C_in: int, H: int, W: int, C_out: int, kernel_size: int, stride: int) -> int:
    """0 when dvmvs_direct_conv_fwd does not take the problem (the caller keeps its library convolution); else the number of
    16-channel output tiles per wave (1 or 2) to pack the weights for."""
    return _capi.lib().dvmvs_direct_conv_tile(int(B), int(C_in), int(H), int(W), int(C_out), int(kernel_size), int(stride))


def direct_conv_pack(weight: Tensor, n_tile: int) -> Tensor:
    """[C_out, C_in, k, k] convolution weights re-packed once into the MFMA B-operand order the kernel streams."""
    _dev_f32("direct_conv_pack", weight)
    C_out, C_in, kh, kw = weight.shape
    nbytes = _capi.lib().dvmvs_direct_conv_packed_bytes(C_out, C_in, kh, int(n_tile)) if kh == kw else 0
    if nbytes == 0:
        raise ValueError(f"dvmvs::direct_conv_pack: need a 3x3 or 5x5 kernel and C_out % (16 * n_tile) == 0, got {tuple(weight.shape)}, n_tile {n_tile}")
    packed = torch.empty(nbytes // 4, dtype=torch.float32, device=weight.device)
    with torch.cuda.device(weight.device):
        rc = _capi.lib().dvmvs_direct_conv_pack(_ptr(weight.contiguous()), _ptr(packed), C_out, C_in, kh, int(n_tile), _stream(weight))
    _capi.check(rc, "dvmvs_direct_conv_pack")
    return packed


def direct_conv_into(x: Tensor, packed: Tensor, n_tile: int, bias, dst: Tensor, C_out: int, kernel_size: int, stride: int, activation: int,
                     dst_nhwc=None) -> Tensor:
    """dst = act(conv2d(x, W, padding = k // 2, stride) + bias) with ``direct_conv_pack``-ed weights; ``dst`` a dense [B,C_out,H/s,W/s]
    tensor or a channel slice of a concatenation buffer; activation "none" or "relu".  ``dst_nhwc``: a second destination that receives the
    same values channels-last ([B,C_out,H/s,W/s] in torch.channels_last memory format), written in the same epilogue."""
    _dev_f32("direct_conv_into", x, packed, dst)
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError("dvmvs::direct_conv_into: expected a contiguous NCHW input")
    B, C_in, H, W = x.shape
    batch_stride = _slice_batch_stride("direct_conv_into", dst, B, int(C_out), H // stride, W // stride)
    if bias is not None and bias.numel() not in (0, C_out):
        raise ValueError(f"dvmvs::direct_conv_into: bias has {bias.numel()} entries for {C_out} channels")
    if dst_nhwc is not None:
        _dev_f32("direct_conv_into", dst_nhwc)
        if tuple(dst_nhwc.shape) != (B, int(C_out), H // stride, W // stride) or not dst_nhwc.is_contiguous(memory_format=torch.channels_last):
            raise ValueError("dvmvs::direct_conv_into: dst_nhwc must be a dense channels-last tensor of the output's shape")
    with torch.cuda.device(x.device):
        rc = _capi.lib().dvmvs_direct_conv_dual_fwd(_ptr(x), 0, _ptr(packed), int(n_tile), _ptr(bias) if bias is not None and bias.numel() else None,
                                                    _ptr(dst), batch_stride, _ptr(dst_nhwc) if dst_nhwc is not None else None, B, C_in, H, W, int(C_out),
                                                    int(kernel_size), int(stride), int(activation), _stream(x))
    _capi.check(rc, "dvmvs_direct_conv_dual_fwd")
    return dst


# ---- 1x1 convolutions (csrc/pointwise_conv.hip): fp32 MFMA GEMM from the NCHW map, bias + ReLU + residual in its store path ----
def pointwise_conv_supported(B: int, C_in: int, H: int, W: int, C_out: int, activation: int, residual_mode: int) -> bool:
    """Whether dvmvs_pointwise_conv_fwd takes the problem (else the caller keeps its library convolution + epilogue launch)."""
    return bool(_capi.lib().dvmvs_pointwise_conv_supported(int(B), int(C_in), int(H), int(W), int(C_out), int(activation), int(residual_mode)))


def pointwise_conv_pack(weight: Tensor) -> Tensor:
    """[C_out,C_in,1,1] (or [C_out,C_in]) -> the kernel's B-operand order; once per layer (the weights are constants at inference)."""
    _dev_f32("pointwise_conv_pack", weight)
    if weight.dim() not in (2, 4) or (weight.dim() == 4 and tuple(weight.shape[2:]) != (1, 1)):
        raise ValueError(f"dvmvs::pointwise_conv_pack: need a [C_out,C_in,1,1] weight, got {tuple(weight.shape)}")
    C_out, C_in = int(weight.shape[0]), int(weight.shape[1])
    nbytes = _capi.lib().dvmvs_pointwise_conv_packed_bytes(C_out, C_in)
    packed = torch.empty(nbytes // 4, device=weight.device, dtype=torch.float32)
    with torch.cuda.device(weight.device):
        rc = _capi.lib().dvmvs_pointwise_conv_pack(_ptr(weight.contiguous()), _ptr(packed), C_out, C_in, _stream(weight))
    _capi.check(rc, "dvmvs_pointwise_conv_pack")
    return packed


def pointwise_conv_into(x: Tensor, packed: Tensor, bias, dst: Tensor, C_out: int, activation: int, residual=None, residual_mode: int = 0,
                        splits: int = 0) -> Tensor:
    """dst = act(conv1x1(x, W) + bias) + residual with ``pointwise_conv_pack``-ed weights; ``dst`` a dense [B,C_out,H,W] tensor or a channel
    slice of a concatenation buffer; activation "none" or "relu"; ``residual`` / ``residual_mode`` as ``bias_act_into`` (1: same shape,
    2: half resolution, nearest-up-sampled)."""
    _dev_f32("pointwise_conv_into", x, packed, dst)
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError("dvmvs::pointwise_conv_into: expected a contiguous NCHW input")
    B, C_in, H, W = x.shape
    C_out = int(C_out)
    if packed.numel() * 4 != _capi.lib().dvmvs_pointwise_conv_packed_bytes(C_out, C_in):
        raise ValueError(f"dvmvs::pointwise_conv_into: the packed weights are not those of a {C_in} -> {C_out} layer")
    batch_stride = _slice_batch_stride("pointwise_conv_into", dst, B, C_out, H, W)
    if bias is not None and bias.numel() not in (0, C_out):
        raise ValueError(f"dvmvs::pointwise_conv_into: bias has {bias.numel()} entries for {C_out} channels")
    residual_stride = 0
    if residual_mode:
        _dev_f32("pointwise_conv_into", residual)
        shape = (B, C_out, H, W) if residual_mode == 1 else (B, C_out, H // 2, W // 2)
        if tuple(residual.shape) != shape:
            raise ValueError(f"dvmvs::pointwise_conv_into: residual of shape {tuple(residual.shape)}, mode {residual_mode} expects {shape}")
        residual_stride = _slice_batch_stride("pointwise_conv_into", residual, *shape)
    with torch.cuda.device(x.device):
        rc = _capi.lib().dvmvs_pointwise_conv_fwd(_ptr(x), 0, _ptr(packed), _ptr(bias) if bias is not None and bias.numel() else None,
                                                  _ptr(residual) if residual_mode else None, residual_stride, int(residual_mode), _ptr(dst), batch_stride,
                                                  B, C_in, H, W, C_out, int(activation), int(splits), _stream(x))
    _capi.check(rc, "dvmvs_pointwise_conv_fwd")
    return dst


def conv_head_into(x: Tensor, weight: Tensor, bias, dst: Tensor, activation: int = 0, p0: float = 0.0, p1: float = 0.0) -> Tensor:
    """3x3, padding 1 convolution with ONE output channel (the decoder's depth heads): dst [B,1,H,W] = act(conv(x, weight) + bias);
    bias None and activation 0: the raw convolution output (the consumer applies bias + activation)."""
    _dev_f32("conv_head_into", x, weight, dst)
    if x.dim() != 4 or not x.is_contiguous() or tuple(weight.shape) != (1, x.shape[1], 3, 3) or not weight.is_contiguous():
        raise ValueError(f"dvmvs::conv_head_into: expected a contiguous NCHW input and a [1,{x.shape[1]},3,3] weight, got {tuple(x.shape)}, {tuple(weight.shape)}")
    B, C_in, H, W = x.shape
    batch_stride = _slice_batch_stride("conv_head_into", dst, B, 1, H, W)
    with torch.cuda.device(x.device):
        rc = _capi.lib().dvmvs_conv_head_fwd(_ptr(x), 0, _ptr(weight), _ptr(bias) if bias is not None and bias.numel() else None, _ptr(dst),
                                             batch_stride, B, C_in, H, W, int(activation), float(p0), float(p1), _stream(x))
    _capi.check(rc, "dvmvs_conv_head_fwd")
    return dst


def lstm_gates_partials_into(conv_partials: Tensor, n_partials: int, c_state: Tensor, h_state: Tensor) -> None:
    """``lstm_gates_into`` on a convolution output that arrives as ``n_partials`` partial sums ([split][B][4*hidden][H*W])."""
    _dev_f32("lstm_gates_partials_into", conv_partials, c_state, h_state)
    B, hidden, H, W = c_state.shape
    if conv_partials.numel() < n_partials * B * 4 * hidden * H * W or tuple(h_state.shape) != tuple(c_state.shape):
        raise ValueError("dvmvs::lstm_gates_partials_into: shapes do not match")
    if not (conv_partials.is_contiguous() and c_state.is_contiguous() and h_state.is_contiguous()):
        raise ValueError("dvmvs::lstm_gates_partials_into: expected contiguous tensors")
    with torch.cuda.device(c_state.device):
        rc = _capi.lib().dvmvs_lstm_gates_partials_fwd(_ptr(conv_partials), int(n_partials), _ptr(c_state), _ptr(h_state), _ptr(c_state), B, hidden, H, W,
                                                       _stream(c_state))
    _capi.check(rc, "dvmvs_lstm_gates_partials_fwd")


def hidden_warp_into(image_src: Tensor, depth_dst: Tensor, src_trans_dst: Tensor, camera_matrix: Tensor, zero_invalid: bool, dst: Tensor) -> Tensor:
    _dev_f32("hidden_warp_into", image_src, depth_dst, src_trans_dst, camera_matrix, dst)
    B, C, H, W = image_src.shape
    if not (image_src.is_contiguous() and dst.is_contiguous() and tuple(dst.shape) == (B, C, H, W)):
        raise ValueError("dvmvs::hidden_warp_into: source and destination must be contiguous [B,C,H,W]")
    with torch.cuda.device(image_src.device):
        rc = _capi.lib().dvmvs_hidden_warp_fwd(_ptr(image_src), _ptr(depth_dst.contiguous()), _ptr(src_trans_dst.contiguous()),
                                               _ptr(camera_matrix.contiguous()), _ptr(dst), B, C, H, W, int(bool(zero_invalid)), _stream(image_src))
    _capi.check(rc, "dvmvs_hidden_warp_fwd")
    return dst


def depth_reproject_lowres_into(transformation: Tensor, previous_depth: Tensor, full_K: Tensor, half_K: Tensor, zbuffer: Tensor, out_lowres: Tensor,
                                factor: int) -> Tensor:
    """Splat + decimate with a caller-owned z-buffer [B,Hf/2,Wf/2] that is all-zero before and after the call (two launches)."""
    _dev_f32("depth_reproject_lowres_into", transformation, previous_depth, full_K, half_K, zbuffer, out_lowres)
    B, one, Hf, Wf = previous_depth.shape
    if one != 1 or zbuffer.numel() != B * (Hf // 2) * (Wf // 2) or not zbuffer.is_contiguous() or not out_lowres.is_contiguous() or \
            out_lowres.numel() != B * ((Hf // 2) // factor) * ((Wf // 2) // factor):
        raise ValueError("dvmvs::depth_reproject_lowres_into: buffer shapes do not match the previous depth")
    with torch.cuda.device(previous_depth.device):
        rc = _capi.lib().dvmvs_depth_reproject_lowres_fwd(_ptr(transformation.contiguous()), _ptr(previous_depth.contiguous()), _ptr(full_K.contiguous()),
                                                          _ptr(half_K.contiguous()), _ptr(zbuffer), _ptr(out_lowres), int(factor), B, Hf, Wf,
                                                          _stream(previous_depth))
    _capi.check(rc, "dvmvs_depth_reproject_lowres_fwd")
    return out_lowres


def depth_reproject_estimate_into(transformation: Tensor, previous_depth: Tensor, full_K: Tensor, half_K: Tensor, estimate: Tensor,
                                  estimate_to_clear: Optional[Tensor], factor: int) -> Tensor:
    """The frame path's re-projection in one launch (dvmvs_depth_reproject_estimate_fwd): splat straight into ``estimate``
    [B,1,H/2/f,W/2/f] (all-zero on entry), zero-filling ``estimate_to_clear`` (the buffer of the frame after next) on the way."""
    _dev_f32("depth_reproject_estimate_into", transformation, previous_depth, full_K, half_K, estimate)
    B, one, Hf, Wf = previous_depth.shape
    shape = (B, 1, Hf // 2 // factor, Wf // 2 // factor)
    if one != 1 or tuple(estimate.shape) != shape or not estimate.is_contiguous() or not previous_depth.is_contiguous() or \
            (estimate_to_clear is not None and (tuple(estimate_to_clear.shape) != shape or not estimate_to_clear.is_contiguous() or
                                                estimate_to_clear.data_ptr() == estimate.data_ptr())):
        raise ValueError("dvmvs::depth_reproject_estimate_into: expected contiguous [B,1,H,W] depth and distinct [B,1,H/2/f,W/2/f] estimate buffers")
    with torch.cuda.device(previous_depth.device):
        rc = _capi.lib().dvmvs_depth_reproject_estimate_fwd(_ptr(transformation.contiguous()), _ptr(previous_depth), _ptr(full_K.contiguous()),
                                                            _ptr(half_K.contiguous()), _ptr(estimate),
                                                            _ptr(estimate_to_clear) if estimate_to_clear is not None else None, int(factor), B, Hf, Wf,
                                                            _stream(previous_depth))
    _capi.check(rc, "dvmvs_depth_reproject_estimate_fwd")
    return estimate


def copy_batch(pairs) -> None:
    """``dst.copy_(src)`` for up to eight (dst, src) pairs of equally laid out dense float32 device tensors in ONE launch (dvmvs_copy_batch).
    The caller guarantees what the C entry requires: same shape and strides per pair, dense storage, 16-byte aligned, a multiple of 4
    elements, no overlap between pairs (``batchable`` checks one pair)."""
    n = len(pairs)
    srcs, dsts, counts = (ctypes.c_void_p * n)(), (ctypes.c_void_p * n)(), (ctypes.c_longlong * n)()
    for j, (dst, src) in enumerate(pairs):
        srcs[j], dsts[j], counts[j] = src.data_ptr(), dst.data_ptr(), dst.numel()
    device = pairs[0][0].device
    with torch.cuda.device(device):
        rc = _capi.lib().dvmvs_copy_batch(srcs, dsts, counts, n, _stream(pairs[0][0]))
    _capi.check(rc, "dvmvs_copy_batch")


def batchable(dst: Tensor, src: Tensor) -> bool:
    """Whether ``dst.copy_(src)`` is a flat copy dvmvs_copy_batch can take."""
    return (dst.is_cuda and src.is_cuda and dst.device == src.device and dst.dtype == torch.float32 and src.dtype == torch.float32
            and dst.shape == src.shape and dst.numel() % 4 == 0 and dst.numel() > 0 and dst.data_ptr() % 16 == 0 and src.data_ptr() % 16 == 0
            and ((dst.is_contiguous() and src.is_contiguous())
                 or (dst.dim() == 4 and dst.is_contiguous(memory_format=torch.channels_last) and src.is_contiguous(memory_format=torch.channels_last))))


def nchw_to_nhwc_into(src: Tensor, dst: Tensor) -> Tensor:
    """``dst`` (a channels-last [B,C,H,W] tensor) = ``src`` (contiguous NCHW), one HIP launch (dvmvs_nchw_to_nhwc: C <= 64, a multiple of 4)."""
    _dev_f32("nchw_to_nhwc_into", src, dst)
    B, C, H, W = src.shape
    if tuple(dst.shape) != (B, C, H, W) or not src.is_contiguous() or not dst.is_contiguous(memory_format=torch.channels_last):
        raise ValueError("dvmvs::nchw_to_nhwc_into: expected a contiguous NCHW source and a channels-last destination of the same shape")
    with torch.cuda.device(src.device):
        rc = _capi.lib().dvmvs_nchw_to_nhwc(_ptr(src), _ptr(dst), B, C, H, W, _stream(src))
    _capi.check(rc, "dvmvs_nchw_to_nhwc")
    return dst


def cost_volume_into(image1: Tensor, image2s, Hm: Tensor, kt: Tensor, min_depth: float, max_depth: float, dst: Tensor, variant: int = 0,
                     work_list: Optional[Tensor] = None) -> Tensor:
    """Dot-product cost volume written into ``dst`` [B,D,H,W] (contiguous: for B == 1 a channel slice of a larger buffer is)."""
    _dev_f32("cost_volume_into", image1, Hm, kt, dst, *image2s)
    B, C, H, W = image1.shape
    M, D = len(image2s), dst.shape[1]
    _check_sweep_matrices("cost_volume_into", Hm, kt, B, M)
    nhwc = C > 1 and all(t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous() for t in image2s)
    if not (image1.is_contiguous() and dst.is_contiguous() and tuple(dst.shape) == (B, D, H, W) and (nhwc or all(t.is_contiguous() for t in image2s))):
        raise ValueError("dvmvs::cost_volume_into: expected contiguous NCHW tensors (measurement maps: all NCHW or all channels-last)")
    workspace, ws_bytes = sweep_workspace(image1.device, B, M, H, W, D) if COST_VOLUME_TWO_PASS else (None, 0)
    items = _work_list_ptr(work_list, image1, B, H, W, D)
    with torch.cuda.device(image1.device):
        rc = _capi.lib().dvmvs_cost_volume_planned_fwd(_ptr(image1), _capi.pointer_array([_ptr(t) for t in image2s]), _ptr(Hm.contiguous()),
                                                       _ptr(kt.contiguous()), _ptr(dst), B, M, C, H, W, D, float(min_depth), float(max_depth), 1, int(variant),
                                                       _capi.LAYOUT_NHWC if nhwc else _capi.LAYOUT_NCHW, _ptr(workspace) if workspace is not None else None, ws_bytes, items, _stream(image1))
    if rc != 0 and workspace is not None:
        drop_sweep_workspace(image1.device, B, M, H, W, D)
    _capi.check(rc, "dvmvs_cost_volume_planned_fwd")
    return dst


# ----------------------------------------------------------------------------------------------------------------------
# baselines (MVDepthNet, GP-MVS): the RGB SAD sweep into the encoder input and GP-MVS's filter step (inference only)
# ----------------------------------------------------------------------------------------------------------------------
@torch.library.custom_op("dvmvs::rgb_sweep", mutates_args=("out",), device_types="cuda")
def rgb_sweep(out: Tensor, image1: Tensor, image2s: Sequence[Tensor], Hm: Tensor, kt: Tensor, min_depth: float, max_depth: float,
              n_depth_levels: int, channel_offset: int, copy_image: bool) -> None:
    """In place: ``out[:, channel_offset:channel_offset + n_depth_levels]`` = the SAD cost volume of the 3-channel ``image1`` against
    ``image2s`` (cost_volume_fusion(..., dot_product=False)); with ``copy_image`` also ``out[:, 0:3] = image1``.  ``out`` is a
    contiguous [B,Cout,H,W] tensor; no other channel is written.  Bit-identical to ``cost_volume(..., dot_product=False, variant=1)``."""
    _dev_f32("rgb_sweep", out, image1, Hm, kt, *image2s)
    M = len(image2s)
    if M == 0:
        raise ValueError("dvmvs::rgb_sweep: need at least one measurement image")
    B, C, H, W = image1.shape
    _check_sweep_matrices("rgb_sweep", Hm, kt, B, M)
    if out.dim() != 4 or not out.is_contiguous() or tuple(out.shape[::2]) != (B, H) or out.shape[3] != W:
        raise ValueError(f"dvmvs::rgb_sweep: expected a contiguous [{B},Cout,{H},{W}] output, got {tuple(out.shape)}")
    for t in image2s:
        if t.shape != image1.shape:
            raise ValueError(f"dvmvs::rgb_sweep: measurement image {tuple(t.shape)} != reference {tuple(image1.shape)}")
    image1 = image1.contiguous()
    image2s = [t.contiguous() for t in image2s]
    with torch.cuda.device(out.device):
        rc = _capi.lib().dvmvs_rgb_sweep_fwd(_ptr(image1), _capi.pointer_array([_ptr(t) for t in image2s]), _ptr(Hm.contiguous()),
                                             _ptr(kt.contiguous()), _ptr(out), B, M, C, H, W, int(n_depth_levels), float(min_depth),
                                             float(max_depth), out.shape[1], int(channel_offset), int(bool(copy_image)), _stream(out))
    _capi.check(rc, "dvmvs_rgb_sweep_fwd")


@rgb_sweep.register_fake
def _(out, image1, image2s, Hm, kt, min_depth, max_depth, n_depth_levels, channel_offset, copy_image):
    return None


@rgb_sweep.register_kernel("cpu")
def _(out, image1, image2s, Hm, kt, min_depth, max_depth, n_depth_levels, channel_offset, copy_image):
    _no_cpu("rgb_sweep")


@torch.library.custom_op("dvmvs::gp_filter_step", mutates_args=("state",), device_types="cuda")
def gp_filter_step(state: Tensor, y: Tensor, A: Sequence[float], k: Sequence[float], reset: bool) -> Tensor:
    """One step of GP-MVS's Kalman filter: ``state`` [2,N] float64 in place (M <- A M; M <- M + k (y - M[0])), returns
    relu(float32(M[0])) shaped like ``y`` (fp32, N elements).  ``A`` = the 2x2 transition row-major, ``k`` the gain (host
    algebra: dvmvs.baselines.runner.GPFilter); ``reset`` starts from M = 0."""
    _dev_f32("gp_filter_step", y)
    if state.device != y.device or state.dtype != torch.float64 or not state.is_contiguous() or tuple(state.shape) != (2, y.numel()):
        raise ValueError(f"dvmvs::gp_filter_step: expected a contiguous float64 state [2,{y.numel()}] on {y.device}, got "
                         f"{state.dtype} {tuple(state.shape)} on {state.device}")
    if len(A) != 4 or len(k) != 2:
        raise ValueError("dvmvs::gp_filter_step: A has 4 entries (row-major 2x2), k has 2")
    y = y.contiguous()
    z = torch.empty_like(y)
    with torch.cuda.device(y.device):
        rc = _capi.lib().dvmvs_gp_filter_step(_ptr(state), _ptr(y), _ptr(z), y.numel(), float(A[0]), float(A[1]), float(A[2]), float(A[3]),
                                              float(k[0]), float(k[1]), int(bool(reset)), _stream(y))
    _capi.check(rc, "dvmvs_gp_filter_step")
    return z


@gp_filter_step.register_fake
def _(state, y, A, k, reset):
    return torch.empty_like(y)


@gp_filter_step.register_kernel("cpu")
def _(state, y, A, k, reset):
    _no_cpu("gp_filter_step")


# ----------------------------------------------------------------------------------------------------------------------
# DPSNet baseline: the plane volume of one measurement frame and the up-sampling soft-argmin (inference only)
# ----------------------------------------------------------------------------------------------------------------------
@torch.library.custom_op("dvmvs::dps_volume", mutates_args=(), device_types="cuda")
def dps_volume(ref: Tensor, meas: Tensor, pose: Tensor, K: Tensor, Kinv: Tensor, nlabel: int, mindepth: float) -> Tensor:
    """[B,2C,nlabel,h,w]: channels 0..C-1 = ``ref`` at every plane, channels C..2C-1 = ``meas`` warped to plane i at depth
    mindepth * nlabel / (i + 1e-16) with DPSNet's ``inverse_warp`` (K^-1 un-projection, Z >= 1e-3, (w - 1) normalisation, coordinates
    outside [-1, 1] fully masked).  ``pose`` [B,3,4] maps the reference camera to the measurement camera; ``K`` / ``Kinv`` [B,3,3] are
    the intrinsics at the resolution of the features."""
    _dev_f32("dps_volume", ref, meas, pose, K, Kinv)
    if ref.dim() != 4 or meas.shape != ref.shape:
        raise ValueError(f"dvmvs::dps_volume: expected two [B,C,h,w] feature maps, got {tuple(ref.shape)} and {tuple(meas.shape)}")
    B, C, h, w = ref.shape
    if tuple(pose.shape) != (B, 3, 4) or tuple(K.shape) != (B, 3, 3) or tuple(Kinv.shape) != (B, 3, 3):
        raise ValueError(f"dvmvs::dps_volume: expected pose [{B},3,4] and K, Kinv [{B},3,3], got {tuple(pose.shape)}, {tuple(K.shape)}, "
                         f"{tuple(Kinv.shape)}")
    ref, meas, pose, K, Kinv = (t.contiguous() for t in (ref, meas, pose, K, Kinv))
    out = torch.empty((B, 2 * C, int(nlabel), h, w), dtype=torch.float32, device=ref.device)
    with torch.cuda.device(ref.device):
        rc = _capi.lib().dvmvs_dps_volume_fwd(_ptr(ref), _ptr(meas), _ptr(pose), _ptr(K), _ptr(Kinv), _ptr(out), B, C, h, w, int(nlabel),
                                              float(mindepth), _stream(ref))
    _capi.check(rc, "dvmvs_dps_volume_fwd")
    return out


@dps_volume.register_fake
def _(ref, meas, pose, K, Kinv, nlabel, mindepth):
    B, C, h, w = ref.shape
    return ref.new_empty((B, 2 * C, nlabel, h, w))


@dps_volume.register_kernel("cpu")
def _(ref, meas, pose, K, Kinv, nlabel, mindepth):
    _no_cpu("dps_volume")


@torch.library.custom_op("dvmvs::dps_regress", mutates_args=(), device_types="cuda")
def dps_regress(costs: Tensor, height: int, width: int, mindepth: float, with_pred: bool = True) -> Tuple[Tensor, Tensor]:
    """(depth [B,1,H,W], pred [B,H,W]) of DPSNet's regression: the plane costs [B,nlabel,h,w] or [B,1,nlabel,h,w] are up-sampled to
    (``height``, ``width``) per plane (bilinear, half-pixel centres), then pred = sum_i softmax_i * i and
    depth = mindepth * nlabel / (pred + 1e-16).  With ``with_pred`` False the expectation is not written (an empty tensor is returned)."""
    _dev_f32("dps_regress", costs)
    if costs.dim() == 5 and costs.shape[1] == 1:
        costs = costs[:, 0]
    if costs.dim() != 4:
        raise ValueError(f"dvmvs::dps_regress: expected costs [B,nlabel,h,w] or [B,1,nlabel,h,w], got {tuple(costs.shape)}")
    costs = costs.contiguous()
    B, nlabel, h, w = costs.shape
    H, W = int(height), int(width)
    depth = torch.empty((B, 1, H, W), dtype=torch.float32, device=costs.device)
    pred = torch.empty((B, H, W) if with_pred else (0,), dtype=torch.float32, device=costs.device)
    with torch.cuda.device(costs.device):
        rc = _capi.lib().dvmvs_dps_regress_fwd(_ptr(costs), _ptr(depth), _ptr(pred) if with_pred else None, B, nlabel, h, w, H, W,
                                               float(mindepth), _stream(costs))
    _capi.check(rc, "dvmvs_dps_regress_fwd")
    return depth, pred


@dps_regress.register_fake
def _(costs, height, width, mindepth, with_pred=True):
    B = costs.shape[0]
    return costs.new_empty((B, 1, height, width)), costs.new_empty((B, height, width) if with_pred else (0,))


@dps_regress.register_kernel("cpu")
def _(costs, height, width, mindepth, with_pred=True):
    _no_cpu("dps_regress")


# ----------------------------------------------------------------------------------------------------------------------
# frame pre-processing: raw 8-bit frames / 16-bit depth maps -> network input, one launch for N frames (inference only)
# ----------------------------------------------------------------------------------------------------------------------
def _raw_frames(name, raw, dtypes, channels):
    """``raw`` as [N,H,W(,3)] on the device with unit element stride inside a row and frames H rows apart; returns (tensor, N, H, W)."""
    if raw.device.type != "cuda":
        _no_cpu(name)
    if raw.dtype not in dtypes:
        raise TypeError(f"dvmvs::{name}: expected {' or '.join(str(d) for d in dtypes)} frames, got {raw.dtype}")
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
    raw, N, H, W = _raw_frames("preprocess_rgb", raw, (torch.uint8,), True)
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
    else:
        _dev_f32("preprocess_rgb", out)
        if out.device != raw.device or tuple(out.shape) != (N, 3, new_height, new_width) or \
                tuple(out.stride()[1:]) != (new_height * new_width, new_width, 1) or (N > 1 and out.stride(0) < frame):
            raise ValueError(f"dvmvs::preprocess_rgb: out must be a float32 [{N},3,{new_height},{new_width}] view on {raw.device} with dense "
                             f"planes, got {tuple(out.shape)} with strides {tuple(out.stride())} on {out.device}")
    batch_stride = out.stride(0) if N > 1 else frame
    with torch.cuda.device(raw.device):
        rc = _capi.lib().dvmvs_preprocess_rgb_fwd(_ptr(raw), _ptr(out), N, H, W, raw.stride(1), crop_x, crop_y, new_height, new_width,
                                                  batch_stride, float(scale) if normalize else 1.0,
                                                  _capi.float_array(mean) if normalize else None,
                                                  _capi.float_array(std) if normalize else None, int(normalize), _stream(raw))
    _capi.check(rc, "dvmvs_preprocess_rgb_fwd")
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
    if out is None:
        out = torch.empty((N, new_height, new_width), dtype=torch.float32, device=raw.device)
    else:
        _dev_f32("preprocess_depth", out)
        if out.device != raw.device or tuple(out.shape) != (N, new_height, new_width) or not out.is_contiguous():
            raise ValueError(f"dvmvs::preprocess_depth: out must be a contiguous float32 [{N},{new_height},{new_width}] tensor on {raw.device}, "
                             f"got {tuple(out.shape)} on {out.device}")
    with torch.cuda.device(raw.device):
        rc = _capi.lib().dvmvs_preprocess_depth_fwd(_ptr(raw), _ptr(out), N, H, W, crop_x, crop_y, new_height, new_width, float(scaling),
                                                    _stream(raw))
    _capi.check(rc, "dvmvs_preprocess_depth_fwd")
    return out


# ----------------------------------------------------------------------------------------------------------------------
# depth evaluation: the eight metrics of dvmvs.errors.compute_errors for N frames, one launch (inference only)
# ----------------------------------------------------------------------------------------------------------------------
_error_workspaces = {}


def depth_errors_workspace(device, n_frames, pixels):
    """Persistent workspace of ``depth_errors`` for (device, N, pixels): zero-filled once here; every call leaves its ticket words zero
    (contract in include/dvmvs_hip.h).  As with ``sweep_workspace``, calls that share it must be ordered with respect to each other (one
    stream per process); allocated outside any graph capture when the first (eager / warm-up) call of a size happens."""
    device = torch.device(device)
    index = device.index if device.index is not None else torch.cuda.current_device()
    key = (index, n_frames, pixels)
    workspace = _error_workspaces.get(key)
    if workspace is None:
        nbytes = _capi.lib().dvmvs_depth_errors_workspace_bytes(n_frames, pixels)
        if nbytes == 0:
            _capi.check(EUNSUPPORTED, "dvmvs_depth_errors_workspace_bytes")
        workspace = torch.zeros((nbytes + 7) // 8, dtype=torch.float64, device=device)
        _error_workspaces[key] = workspace
    return workspace


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
    if gt.device.type != "cuda" or pred.device.type != "cuda":
        _no_cpu("depth_errors")
    if gt.dtype != torch.float32 or pred.dtype != torch.float32:
        raise ValueError(f"dvmvs::depth_errors: expected float32 depth maps, got {gt.dtype} and {pred.dtype}")
    N, pixels = _frames_2d("depth_errors", gt)
    if _frames_2d("depth_errors", pred) != (N, pixels) or tuple(gt.shape[-2:]) != tuple(pred.shape[-2:]) or gt.device != pred.device:
        raise ValueError(f"dvmvs::depth_errors: gt {tuple(gt.shape)} on {gt.device} and pred {tuple(pred.shape)} on {pred.device} differ")
    if N < 1 or pixels < 1:
        raise ValueError(f"dvmvs::depth_errors: expected non-empty depth maps, got {tuple(gt.shape)}")
    max_depth = float(max_depth)
    if max_depth != max_depth:
        raise ValueError("dvmvs::depth_errors: max_depth is NaN")
    gt, pred = gt.contiguous(), pred.contiguous()
    if out is None:
        out = torch.empty((N, 8), dtype=torch.float32, device=gt.device)
    elif out.device != gt.device or out.dtype != torch.float32 or tuple(out.shape) != (N, 8) or not out.is_contiguous():
        raise ValueError(f"dvmvs::depth_errors: out must be a contiguous float32 [{N},8] tensor on {gt.device}, got {out.dtype} "
                         f"{tuple(out.shape)} on {out.device}")
    if counts is not None and (counts.device != gt.device or counts.dtype != torch.int32 or tuple(counts.shape) != (N, 4)
                               or not counts.is_contiguous()):
        raise ValueError(f"dvmvs::depth_errors: counts must be a contiguous int32 [{N},4] tensor on {gt.device}, got {counts.dtype} "
                         f"{tuple(counts.shape)} on {counts.device}")
    workspace = depth_errors_workspace(gt.device, N, pixels)
    with torch.cuda.device(gt.device):
        rc = _capi.lib().dvmvs_depth_errors_fwd(_ptr(gt), _ptr(pred), N, pixels, max_depth, _ptr(out),
                                                _ptr(counts) if counts is not None else None, _ptr(workspace), _stream(gt))
    _capi.check(rc, "dvmvs_depth_errors_fwd")
    return out


# ----------------------------------------------------------------------------------------------------------------------
# ray-casting a fused TSDF volume from camera views (inference only)
# ----------------------------------------------------------------------------------------------------------------------
def _raycast_volumes(name, tsdf, weight, color=None):
    for label, t in (("tsdf", tsdf), ("weight", weight), ("color", color)):
        if t is None:
            continue
        if t.device.type != "cuda":
            _no_cpu(name)
        if t.dtype != torch.float32 or t.dim() != 3 or t.shape != tsdf.shape or t.device != tsdf.device or not t.is_contiguous():
            raise ValueError(f"dvmvs::{name}: {label} must be a contiguous float32 [X,Y,Z] tensor like tsdf {tuple(tsdf.shape)} on "
                             f"{tsdf.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    X, Y, Z = (int(d) for d in tsdf.shape)
    if min(X, Y, Z) < 2:
        raise ValueError(f"dvmvs::{name}: every dimension of the volume must be at least 2, got {X}x{Y}x{Z}")
    return X, Y, Z


def tsdf_raycast_mask(tsdf: Tensor, weight: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """Brick mask of a TSDF volume for ``tsdf_raycast``: uint8 [ceil((X-1)/8), ceil((Y-1)/8), ceil((Z-1)/8)], 1 where one of the brick's
    8x8x8 cells has a corner with ``weight > 0 and tsdf <= 0``.  It describes the volume's CURRENT contents: rebuild it after every
    change.  ``out``: a contiguous uint8 tensor of that shape; it is returned."""
    X, Y, Z = _raycast_volumes("tsdf_raycast_mask", tsdf, weight)
    shape = ((X + 6) // 8, (Y + 6) // 8, (Z + 6) // 8)
    nbytes = _capi.lib().dvmvs_tsdf_raycast_mask_bytes(X, Y, Z)
    if nbytes == 0:
        _capi.check(EUNSUPPORTED, "dvmvs_tsdf_raycast_mask_bytes")
    assert nbytes == shape[0] * shape[1] * shape[2]
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=tsdf.device)
    elif out.device != tsdf.device or out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError(f"dvmvs::tsdf_raycast_mask: out must be a contiguous uint8 {shape} tensor on {tsdf.device}, got {out.dtype} "
                         f"{tuple(out.shape)} on {out.device}")
    with torch.cuda.device(tsdf.device):
        rc = _capi.lib().dvmvs_tsdf_raycast_mask(_ptr(tsdf), _ptr(weight), X, Y, Z, _ptr(out), _stream(tsdf))
    _capi.check(rc, "dvmvs_tsdf_raycast_mask")
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
    X, Y, Z = _raycast_volumes("tsdf_raycast", tsdf, weight, color)
    dev = tsdf.device
    if colour and color is None:
        raise ValueError("dvmvs::tsdf_raycast: colour output needs the colour volume")
    for label, t, tail in (("cam_intr", cam_intr, (3, 3)), ("cam_pose", cam_pose, (4, 4))):
        if t.device.type != "cuda":
            _no_cpu("tsdf_raycast")
        if t.dtype != torch.float32 or t.dim() != 3 or tuple(t.shape[1:]) != tail or t.device != dev:
            raise ValueError(f"dvmvs::tsdf_raycast: {label} must be float32 [N,{tail[0]},{tail[1]}] on {dev}, got {t.dtype} "
                             f"{tuple(t.shape)} on {t.device}")
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
    if mask is not None:
        shape = ((X + 6) // 8, (Y + 6) // 8, (Z + 6) // 8)
        if mask.device != dev or mask.dtype != torch.uint8 or tuple(mask.shape) != shape or not mask.is_contiguous():
            raise ValueError(f"dvmvs::tsdf_raycast: mask must be the contiguous uint8 {shape} tensor of tsdf_raycast_mask on {dev}, got "
                             f"{mask.dtype} {tuple(mask.shape)} on {mask.device}")
    cam_intr, cam_pose = cam_intr.contiguous(), cam_pose.contiguous()
    depth = torch.empty((N, height, width), dtype=torch.float32, device=dev)
    normal = torch.empty((N, height, width, 3), dtype=torch.float32, device=dev) if normals else None
    rgb = torch.empty((N, height, width, 3), dtype=torch.uint8, device=dev) if colour else None
    with torch.cuda.device(dev):
        rc = _capi.lib().dvmvs_tsdf_raycast_fwd(
            _ptr(tsdf), _ptr(weight), None if color is None else _ptr(color), X, Y, Z, origin[0], origin[1], origin[2], voxel_size,
            None if mask is None else _ptr(mask), _ptr(cam_intr), _ptr(cam_pose), N, height, width, near, far, step, _ptr(depth),
            None if normal is None else _ptr(normal), None if rgb is None else _ptr(rgb), _stream(tsdf))
    _capi.check(rc, "dvmvs_tsdf_raycast_fwd")
    return depth, normal, rgb


# ----------------------------------------------------------------------------------------------------------------------
# fusing a batch of frames into a TSDF volume: one pass over the volume, the bits of per-frame integration (inference only)
# ----------------------------------------------------------------------------------------------------------------------
_fuse_workspaces = {}
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
    device = torch.device(device)
    index = device.index if device.index is not None else torch.cuda.current_device()
    workspace = _fuse_workspaces.get(index)
    nbytes = _capi.lib().dvmvs_tsdf_integrate_frames_workspace_bytes(n_frames)
    if workspace is None or workspace.numel() * 4 < nbytes:
        workspace = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)
        _fuse_workspaces[index] = workspace
    return workspace


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
    if (rgb_u8 is None) == (folded is None):
        raise ValueError("dvmvs::tsdf_integrate_frames: exactly one of rgb_u8 and folded must be given")
    tensors = [("tsdf", tsdf), ("weight", weight), ("color", color), ("cam_intr", cam_intr), ("cam_pose", cam_pose), ("depth", depth),
               ("rgb_u8", rgb_u8) if rgb_u8 is not None else ("folded", folded)]
    for label, t in tensors:
        if not torch.is_tensor(t):
            raise TypeError(f"dvmvs::tsdf_integrate_frames: {label} must be a tensor, got {type(t).__name__}")
    if depth.dim() != 3 or depth.dtype != torch.float32:
        raise ValueError(f"dvmvs::tsdf_integrate_frames: depth must be float32 [N,h,w], got {depth.dtype} {tuple(depth.shape)}")
    N, h, w = (int(d) for d in depth.shape)
    if N < 1 or h < 1 or w < 1:
        raise ValueError(f"dvmvs::tsdf_integrate_frames: expected at least one non-empty frame, got depth {tuple(depth.shape)}")
    for label, t in tensors[:3]:
        if t.dtype != torch.float32 or t.dim() != 3 or t.shape != tsdf.shape or t.numel() == 0:
            raise ValueError(f"dvmvs::tsdf_integrate_frames: {label} must be a non-empty float32 [X,Y,Z] tensor like tsdf "
                             f"{tuple(tsdf.shape)}, got {t.dtype} {tuple(t.shape)}")
    for label, t, tail in (("cam_intr", cam_intr, (N, 3, 3)), ("cam_pose", cam_pose, (N, 4, 4))):
        if t.dtype != torch.float32 or tuple(t.shape) != tail:
            raise ValueError(f"dvmvs::tsdf_integrate_frames: {label} must be float32 {list(tail)} for {N} frames, got {t.dtype} {tuple(t.shape)}")
    if rgb_u8 is not None and (rgb_u8.dtype != torch.uint8 or tuple(rgb_u8.shape) != (N, h, w, 3)):
        raise ValueError(f"dvmvs::tsdf_integrate_frames: rgb_u8 must be uint8 [{N},{h},{w},3] like depth, got {rgb_u8.dtype} {tuple(rgb_u8.shape)}")
    if folded is not None and (folded.dtype != torch.float32 or tuple(folded.shape) != (N, h, w)):
        raise ValueError(f"dvmvs::tsdf_integrate_frames: folded must be float32 [{N},{h},{w}] like depth, got {folded.dtype} {tuple(folded.shape)}")
    if hasattr(obs_weight, "tolist"):       # a numpy array or a tensor (one download, not one per element): a 0-d one becomes a number
        obs_weight = obs_weight.tolist()
    weights = [float(x) for x in obs_weight] if isinstance(obs_weight, (list, tuple)) else [float(obs_weight)] * N
    if len(weights) != N:
        raise ValueError(f"dvmvs::tsdf_integrate_frames: {len(weights)} observation weights for {N} frames")
    voxel_size, max_depth = float(voxel_size), float(max_depth)
    trunc_margin = 5.0 * voxel_size if trunc_margin is None else float(trunc_margin)
    if not voxel_size > 0.0 or not trunc_margin > 0.0 or max_depth != max_depth:
        raise ValueError(f"dvmvs::tsdf_integrate_frames: voxel_size and trunc_margin must be positive and max_depth not NaN, got "
                         f"{voxel_size}, {trunc_margin}, {max_depth}")
    origin = [float(o) for o in origin]
    if len(origin) != 3:
        raise ValueError("dvmvs::tsdf_integrate_frames: origin must have three components")
    dev = tsdf.device
    for label, t in tensors:
        if t.device.type != "cuda":
            _no_cpu("tsdf_integrate_frames")
        if t.device != dev or not t.is_contiguous():
            raise ValueError(f"dvmvs::tsdf_integrate_frames: {label} must be contiguous and on {dev} like tsdf (got {t.device}, "
                             f"contiguous={t.is_contiguous()})")
    counters = None
    if torch.is_tensor(stats):
        if stats.device != dev or stats.dtype != torch.int64 or tuple(stats.shape) != (2,) or not stats.is_contiguous():
            raise ValueError(f"dvmvs::tsdf_integrate_frames: stats must be a contiguous int64 [2] tensor on {dev}")
        counters = stats
    elif stats:
        counters = torch.zeros(2, dtype=torch.int64, device=dev)
    X, Y, Z = (int(d) for d in tsdf.shape)
    workspace = tsdf_integrate_frames_workspace(dev, N)
    with torch.cuda.device(dev):
        rc = _capi.lib().dvmvs_tsdf_integrate_frames(
            _ptr(tsdf), _ptr(weight), _ptr(color), X, Y, Z, origin[0], origin[1], origin[2], voxel_size, _ptr(cam_intr), _ptr(cam_pose),
            None if rgb_u8 is None else _ptr(rgb_u8), None if folded is None else _ptr(folded), _ptr(depth), N, h, w, trunc_margin,
            _capi.float_array(weights), max_depth, _ptr(workspace), None if counters is None else _ptr(counters), _stream(tsdf))
    _capi.check(rc, "dvmvs_tsdf_integrate_frames")
    return counters


# ----------------------------------------------------------------------------------------------------------------------
# exact nearest-point distances between point clouds, and the 3-D reconstruction metrics they reduce to (inference only)
# ----------------------------------------------------------------------------------------------------------------------
_nearest_workspaces = {}


def _grown_workspace(key, device, nbytes):
    """The persistent buffer of ``key`` on ``device`` with room for ``nbytes``: grown to the largest request seen, never initialised.  A
    buffer that is replaced is marked as in use on the current stream, so the allocator does not hand its memory out again before the
    work enqueued there has read it."""
    workspace = _nearest_workspaces.get(key)
    if workspace is None or workspace.numel() < nbytes:
        if workspace is not None:
            workspace.record_stream(torch.cuda.current_stream(device))
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _nearest_workspaces[key] = workspace
    return workspace


def nearest_distance_workspace(device, M):
    """Persistent grid workspace of ``nearest_build`` per device: grown to the largest target cloud seen (its size follows from ``M`` alone)
    and written by every build before a query reads it, so it needs no initialisation.  A build overwrites the grid of the build before
    it: calls that share the workspace must be ordered with respect to each other (one stream per process), and a grid that has to
    outlive the next build needs a buffer of its own (``nearest_build(target, workspace=...)``)."""
    device = torch.device(device)
    index = device.index if device.index is not None else torch.cuda.current_device()
    nbytes = _capi.lib().dvmvs_nearest_workspace_bytes(int(M))
    if nbytes == 0:
        raise ValueError(f"dvmvs::nearest_distance: a target cloud of {M} points is outside what the kernels take (1 .. 2^28)")
    return _grown_workspace(("grid", index), device, nbytes)


def _points(name, label, t):
    if not torch.is_tensor(t):
        raise TypeError(f"dvmvs::{name}: {label} must be a tensor, got {type(t).__name__}")
    if t.device.type != "cuda":
        _no_cpu(name)
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"dvmvs::{name}: {label} must be float32 [n,3] points, got {t.dtype} {tuple(t.shape)}")
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
    elif (not torch.is_tensor(workspace) or workspace.device != target.device or workspace.dtype != torch.uint8 or not workspace.is_contiguous()
          or workspace.numel() < _capi.lib().dvmvs_nearest_workspace_bytes(M)):
        raise ValueError(f"dvmvs::nearest_build: workspace must be a contiguous uint8 tensor on {target.device} of at least "
                         f"{_capi.lib().dvmvs_nearest_workspace_bytes(M)} bytes")
    with torch.cuda.device(target.device):
        rc = _capi.lib().dvmvs_nearest_build(_ptr(target), M, _ptr(workspace), workspace.numel(), _stream(target))
    _capi.check(rc, "dvmvs_nearest_build")
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
        dev_index = query.device.index if query.device.index is not None else torch.cuda.current_device()
        scratch = _grown_workspace(("query", dev_index), query.device, _capi.lib().dvmvs_nearest_query_workspace_bytes(N, M))
        with torch.cuda.device(query.device):
            rc = _capi.lib().dvmvs_nearest_distance_fwd(_ptr(query), N, _ptr(target), M, _ptr(workspace), _ptr(scratch), scratch.numel(),
                                                        _ptr(dist), None if index is None else _ptr(index), _stream(query))
        _capi.check(rc, "dvmvs_nearest_distance_fwd")
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
        if not torch.is_tensor(t):
            raise TypeError(f"dvmvs::distance_metrics: {label} must be a tensor, got {type(t).__name__}")
        if t.device.type != "cuda":
            _no_cpu("distance_metrics")
        if t.dtype != torch.float32 or t.dim() != 1 or t.numel() < 1:
            raise ValueError(f"dvmvs::distance_metrics: {label} must be a non-empty float32 [n] tensor, got {t.dtype} {tuple(t.shape)}")
    dev = dist_pred.device
    threshold = float(threshold)
    if dist_gt.device != dev or threshold != threshold:
        raise ValueError(f"dvmvs::distance_metrics: both arrays must be on one device and the threshold not NaN, got {dev}, {dist_gt.device}, "
                         f"{threshold}")
    dist_pred, dist_gt = dist_pred.contiguous(), dist_gt.contiguous()
    if out is None:
        out = torch.empty(6, dtype=torch.float32, device=dev)
    elif out.device != dev or out.dtype != torch.float32 or tuple(out.shape) != (6,) or not out.is_contiguous():
        raise ValueError(f"dvmvs::distance_metrics: out must be a contiguous float32 [6] tensor on {dev}")
    if counts is not None and (counts.device != dev or counts.dtype != torch.int64 or tuple(counts.shape) != (2,) or not counts.is_contiguous()):
        raise ValueError(f"dvmvs::distance_metrics: counts must be a contiguous int64 [2] tensor on {dev}")
    with torch.cuda.device(dev):
        rc = _capi.lib().dvmvs_distance_metrics_fwd(_ptr(dist_pred), dist_pred.numel(), _ptr(dist_gt), dist_gt.numel(), threshold, _ptr(out),
                                                    None if counts is None else _ptr(counts), _stream(dist_pred))
    _capi.check(rc, "dvmvs_distance_metrics_fwd")
    return out


# ----------------------------------------------------------------------------------------------------------------------
# filtering depth maps by multi-view geometric consistency (inference only)
# ----------------------------------------------------------------------------------------------------------------------
CONSISTENCY_MAX_SOURCES = 16


def _consistency_cameras(name, K, poses, sources):
    """Checks types and shapes of the camera tensors of the two consistency ops; returns (N, S)."""
    for label, t in (("K", K), ("poses", poses), ("sources", sources)):
        if not torch.is_tensor(t):
            raise TypeError(f"dvmvs::{name}: {label} must be a tensor, got {type(t).__name__}")
    if K.dtype != torch.float32 or K.dim() != 3 or tuple(K.shape[1:]) != (3, 3) or K.shape[0] < 1:
        raise ValueError(f"dvmvs::{name}: K must be float32 [N,3,3], got {K.dtype} {tuple(K.shape)}")
    N = int(K.shape[0])
    if poses.dtype != torch.float32 or tuple(poses.shape) != (N, 4, 4):
        raise ValueError(f"dvmvs::{name}: poses must be float32 [{N},4,4] camera-to-world, got {poses.dtype} {tuple(poses.shape)}")
    if sources.dtype != torch.int32 or sources.dim() != 2 or sources.shape[0] != N or sources.shape[1] > CONSISTENCY_MAX_SOURCES:
        raise ValueError(f"dvmvs::{name}: sources must be int32 [{N},S] with S <= {CONSISTENCY_MAX_SOURCES}, got {sources.dtype} "
                         f"{tuple(sources.shape)}")
    if N > 65535:
        raise ValueError(f"dvmvs::{name}: at most 65535 frames per call, got {N}")
    return N, int(sources.shape[1])


def _consistency_devices(name, **tensors):
    """Every tensor on the GPU, and on the same one."""
    first = None
    for label, t in tensors.items():
        if t.device.type != "cuda":
            _no_cpu(name)
        first = t.device if first is None else first
        if t.device != first:
            raise ValueError(f"dvmvs::{name}: {label} is on {t.device}, not on {first} like the other tensors")


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
    with torch.cuda.device(K.device):
        rc = _capi.lib().dvmvs_consistency_matrices(_ptr(K), _ptr(poses), _ptr(sources), _ptr(out), N, S, _stream(K))
    _capi.check(rc, "dvmvs_consistency_matrices")
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
    if not torch.is_tensor(depths):
        raise TypeError(f"dvmvs::{name}: depths must be a tensor, got {type(depths).__name__}")
    N, S = _consistency_cameras(name, K, poses, sources)
    if depths.dtype != torch.float32 or depths.dim() != 3 or depths.shape[0] != N or depths.shape[1] < 1 or depths.shape[2] < 1:
        raise ValueError(f"dvmvs::{name}: depths must be non-empty float32 [{N},H,W] like K, got {depths.dtype} {tuple(depths.shape)}")
    H, W = int(depths.shape[1]), int(depths.shape[2])
    if 3 * H * W >= 2 ** 31:
        raise ValueError(f"dvmvs::{name}: a {H}x{W} map is too large (3 H W must stay below 2^31)")
    pixel_threshold, relative_threshold, min_views = float(pixel_threshold), float(relative_threshold), int(min_views)
    if pixel_threshold != pixel_threshold or relative_threshold != relative_threshold:
        raise ValueError(f"dvmvs::{name}: a threshold is NaN")
    if min_views < 0:
        raise ValueError(f"dvmvs::{name}: min_views must not be negative, got {min_views}")
    _consistency_devices(name, depths=depths, K=K, poses=poses, sources=sources)
    if matrices is None:
        matrices = consistency_matrices(K, poses, sources)
    elif (not torch.is_tensor(matrices) or matrices.device != depths.device or matrices.dtype != torch.float32
          or tuple(matrices.shape) != (N, S, 2, 12) or not matrices.is_contiguous()):
        raise ValueError(f"dvmvs::{name}: matrices must be the contiguous float32 [{N},{S},2,12] tensor of consistency_matrices on {depths.device}")
    if out is None:
        out = torch.empty((N, H, W), dtype=torch.float32, device=depths.device)
    elif (not torch.is_tensor(out) or out.device != depths.device or out.dtype != torch.float32 or tuple(out.shape) != (N, H, W)
          or not out.is_contiguous()):
        raise ValueError(f"dvmvs::{name}: out must be a contiguous float32 [{N},{H},{W}] tensor on {depths.device}")
    depths, K, poses, sources = depths.contiguous(), K.contiguous(), poses.contiguous(), sources.contiguous()
    count = torch.empty((N, H, W), dtype=torch.uint8, device=depths.device) if with_count else None
    points = torch.empty((N, H, W, 3), dtype=torch.float32, device=depths.device) if with_points else None
    with torch.cuda.device(depths.device):
        rc = _capi.lib().dvmvs_depth_consistency_fwd(
            _ptr(depths), _ptr(K), _ptr(poses), _ptr(sources), _ptr(matrices), _ptr(out), None if count is None else _ptr(count),
            None if points is None else _ptr(points), N, S, H, W, pixel_threshold, relative_threshold, min_views, 1 if average else 0,
            _stream(depths))
    _capi.check(rc, "dvmvs_depth_consistency_fwd")
    return out, count, points

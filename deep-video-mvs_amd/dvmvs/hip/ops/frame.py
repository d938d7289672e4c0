"""The ops of the frame path: hidden-state warp, ConvLSTM gates, depth re-projection, bias / activation epilogues, up-sampling, depthwise
convolutions (with their training forms) and the destination-passing shims over the convolution kernels."""
import ctypes
from typing import Optional, Tuple

import torch
from torch import Tensor

from dvmvs.hip import _capi
from dvmvs.hip.ops._common import EUNSUPPORTED, channel_ptr, check_tensors, custom_op, launch, opt_ptr, ptr

ACTIVATIONS = {"none": 0, "relu": 1, "sigmoid": 2}
ACTIVATION_SIGMOID_TO_DEPTH = 3
RESIDUAL_NONE, RESIDUAL_SAME, RESIDUAL_NEAREST_UP2 = 0, 1, 2


# ----------------------------------------------------------------------------------------------------------------------
# hidden-state warp
# ----------------------------------------------------------------------------------------------------------------------
def _check_hidden_warp(name, image_src, depth_dst, src_trans_dst, camera_matrix, dst=None):
    """The kernel indexes depth, transform and intrinsics by the SOURCE's batch and map size: all of them (and the destination) must
    have it.  Every malformed argument is reported before a misplaced one, and nothing is launched."""
    check_tensors(name, image_src, label="image_src", shape=(None, None, None, None), on_gpu=False)
    B, C, H, W = image_src.shape
    check_tensors(name, depth_dst, label="depth_dst", shape=(B, 1, H, W), on_gpu=False)
    check_tensors(name, src_trans_dst, label="src_trans_dst", shape=(B, 4, 4), on_gpu=False)
    check_tensors(name, camera_matrix, label="camera_matrix", shape=(B, 3, 3), on_gpu=False)
    if dst is not None:
        check_tensors(name, dst, label="dst", shape=(B, C, H, W), on_gpu=False)
    check_tensors(name, image_src, depth_dst, src_trans_dst, camera_matrix, *(() if dst is None else (dst,)))
    return B, C, H, W


@custom_op("hidden_warp", fake=lambda image_src, depth_dst, src_trans_dst, camera_matrix, zero_invalid: torch.empty_like(image_src))
def hidden_warp(image_src: Tensor, depth_dst: Tensor, src_trans_dst: Tensor, camera_matrix: Tensor,
                zero_invalid: bool) -> Tensor:
    B, C, H, W = _check_hidden_warp("hidden_warp", image_src, depth_dst, src_trans_dst, camera_matrix)
    image_src = image_src.contiguous()
    out = torch.empty_like(image_src)
    launch("dvmvs_hidden_warp_fwd", image_src.device, ptr(image_src), ptr(depth_dst.contiguous()), ptr(src_trans_dst.contiguous()),
           ptr(camera_matrix.contiguous()), ptr(out), B, C, H, W, int(bool(zero_invalid)))
    return out


def _hidden_warp_setup(ctx, inputs, output):
    image_src, depth_dst, src_trans_dst, camera_matrix, _ = inputs
    ctx.shape = tuple(image_src.shape)
    ctx.save_for_backward(depth_dst, src_trans_dst, camera_matrix)


def _hidden_warp_backward(ctx, grad):
    depth_dst, src_trans_dst, camera_matrix = ctx.saved_tensors
    B, C, H, W = ctx.shape
    grad = grad.contiguous()
    gsrc = torch.zeros_like(grad)
    # the validity mask is NOT applied to the gradient, as in the reference (convlstm.py:41 edits .data)
    launch("dvmvs_hidden_warp_bwd", grad.device, ptr(grad), ptr(depth_dst.contiguous()), ptr(src_trans_dst.contiguous()),
           ptr(camera_matrix.contiguous()), ptr(gsrc), B, C, H, W)
    return gsrc, None, None, None, None


torch.library.register_autograd("dvmvs::hidden_warp", _hidden_warp_backward, setup_context=_hidden_warp_setup)


def hidden_warp_into(image_src: Tensor, depth_dst: Tensor, src_trans_dst: Tensor, camera_matrix: Tensor, zero_invalid: bool, dst: Tensor) -> Tensor:
    B, C, H, W = _check_hidden_warp("hidden_warp_into", image_src, depth_dst, src_trans_dst, camera_matrix, dst)
    if not (image_src.is_contiguous() and dst.is_contiguous()):
        raise ValueError("dvmvs::hidden_warp_into: source and destination must be contiguous [B,C,H,W]")
    launch("dvmvs_hidden_warp_fwd", image_src.device, ptr(image_src), ptr(depth_dst.contiguous()), ptr(src_trans_dst.contiguous()),
           ptr(camera_matrix.contiguous()), ptr(dst), B, C, H, W, int(bool(zero_invalid)))
    return dst


# ----------------------------------------------------------------------------------------------------------------------
# ConvLSTM gate fusion
# ----------------------------------------------------------------------------------------------------------------------
@custom_op("lstm_gates", fake=lambda combined_conv, c_cur: (torch.empty_like(c_cur), torch.empty_like(c_cur)))
def lstm_gates(combined_conv: Tensor, c_cur: Tensor) -> Tuple[Tensor, Tensor]:
    check_tensors("lstm_gates", combined_conv, c_cur)
    B, hidden, H, W = c_cur.shape
    if combined_conv.shape != (B, 4 * hidden, H, W):
        raise ValueError(f"dvmvs::lstm_gates: conv output {tuple(combined_conv.shape)} does not match state {tuple(c_cur.shape)}")
    combined_conv, c_cur = combined_conv.contiguous(), c_cur.contiguous()
    h_next, c_next = torch.empty_like(c_cur), torch.empty_like(c_cur)
    launch("dvmvs_lstm_gates_fwd", c_cur.device, ptr(combined_conv), ptr(c_cur), ptr(h_next), ptr(c_next), B, hidden, H, W)
    return h_next, c_next


def _lstm_gates_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)


def _lstm_gates_backward(ctx, grad_h, grad_c):
    combined_conv, c_cur = ctx.saved_tensors
    B, hidden, H, W = c_cur.shape
    cc, cs = combined_conv.contiguous(), c_cur.contiguous()
    gh = grad_h.contiguous() if grad_h is not None else None
    gc = grad_c.contiguous() if grad_c is not None else None
    grad_cc, grad_cs = torch.empty_like(cc), torch.empty_like(cs)
    launch("dvmvs_lstm_gates_bwd", cs.device, opt_ptr(gh), opt_ptr(gc), ptr(cc), ptr(cs), ptr(grad_cc), ptr(grad_cs), B, hidden, H, W)
    return grad_cc, grad_cs


torch.library.register_autograd("dvmvs::lstm_gates", _lstm_gates_backward, setup_context=_lstm_gates_setup)


def lstm_gates_into(combined_conv: Tensor, c_state: Tensor, h_state: Tensor) -> None:
    """State update in place: c_state <- c', h_state <- h' (the kernel reads a row of c completely before it writes it)."""
    check_tensors("lstm_gates_into", combined_conv, c_state, h_state)
    B, hidden, H, W = c_state.shape
    if tuple(combined_conv.shape) != (B, 4 * hidden, H, W) or tuple(h_state.shape) != tuple(c_state.shape):
        raise ValueError("dvmvs::lstm_gates_into: shapes do not match")
    if not (combined_conv.is_contiguous() and c_state.is_contiguous() and h_state.is_contiguous()):
        raise ValueError("dvmvs::lstm_gates_into: expected contiguous tensors")
    launch("dvmvs_lstm_gates_fwd", c_state.device, ptr(combined_conv), ptr(c_state), ptr(h_state), ptr(c_state), B, hidden, H, W)


def lstm_gates_partials_into(conv_partials: Tensor, n_partials: int, c_state: Tensor, h_state: Tensor) -> None:
    """``lstm_gates_into`` on a convolution output that arrives as ``n_partials`` partial sums ([split][B][4*hidden][H*W])."""
    check_tensors("lstm_gates_partials_into", conv_partials, c_state, h_state)
    B, hidden, H, W = c_state.shape
    if conv_partials.numel() < n_partials * B * 4 * hidden * H * W or tuple(h_state.shape) != tuple(c_state.shape):
        raise ValueError("dvmvs::lstm_gates_partials_into: shapes do not match")
    if not (conv_partials.is_contiguous() and c_state.is_contiguous() and h_state.is_contiguous()):
        raise ValueError("dvmvs::lstm_gates_partials_into: expected contiguous tensors")
    launch("dvmvs_lstm_gates_partials_fwd", c_state.device, ptr(conv_partials), int(n_partials), ptr(c_state), ptr(h_state), ptr(c_state),
           B, hidden, H, W)


# ----------------------------------------------------------------------------------------------------------------------
# depth re-projection (forward splat)
# ----------------------------------------------------------------------------------------------------------------------
def _reproject(name, transformation, previous_depth, full_K, half_K, factor):
    check_tensors(name, transformation, previous_depth, full_K, half_K)
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
    launch("dvmvs_depth_reproject_fwd", previous_depth.device, *[ptr(t) for t in args], ptr(out), opt_ptr(low), int(factor), B, Hf, Wf)
    return out, low


def _reproject_fake(transformation, previous_depth, full_K, half_K):
    B, _, Hf, Wf = previous_depth.shape
    return previous_depth.new_empty((B, 1, Hf // 2, Wf // 2))


@custom_op("depth_reproject", fake=_reproject_fake)
def depth_reproject(transformation: Tensor, previous_depth: Tensor, full_K: Tensor, half_K: Tensor) -> Tensor:
    """``transformation`` [B,4,4] = inverse(reference_pose) @ measurement_pose (dvmvs.pose_algebra.relative_pose)."""
    return _reproject("depth_reproject", transformation, previous_depth, full_K, half_K, 0)[0]


def _reproject_lowres_fake(transformation, previous_depth, full_K, half_K, factor):
    B, _, Hf, Wf = previous_depth.shape
    return (previous_depth.new_empty((B, 1, Hf // 2, Wf // 2)),
            previous_depth.new_empty((B, 1, (Hf // 2) // factor, (Wf // 2) // factor)))


@custom_op("depth_reproject_lowres", fake=_reproject_lowres_fake)
def depth_reproject_lowres(transformation: Tensor, previous_depth: Tensor, full_K: Tensor, half_K: Tensor,
                           factor: int) -> Tuple[Tensor, Tensor]:
    """Splat plus the nearest /factor decimation the fusionnet call site applies next (one C-ABI call)."""
    if factor <= 0:
        raise ValueError("dvmvs::depth_reproject_lowres: factor must be positive")
    out, low = _reproject("depth_reproject_lowres", transformation, previous_depth, full_K, half_K, factor)
    return out, low


def depth_reproject_lowres_into(transformation: Tensor, previous_depth: Tensor, full_K: Tensor, half_K: Tensor, zbuffer: Tensor, out_lowres: Tensor,
                                factor: int) -> Tensor:
    """Splat + decimate with a caller-owned z-buffer [B,Hf/2,Wf/2] that is all-zero before and after the call (two launches)."""
    check_tensors("depth_reproject_lowres_into", transformation, previous_depth, full_K, half_K, zbuffer, out_lowres)
    B, one, Hf, Wf = previous_depth.shape
    if one != 1 or zbuffer.numel() != B * (Hf // 2) * (Wf // 2) or not zbuffer.is_contiguous() or not out_lowres.is_contiguous() or \
            out_lowres.numel() != B * ((Hf // 2) // factor) * ((Wf // 2) // factor):
        raise ValueError("dvmvs::depth_reproject_lowres_into: buffer shapes do not match the previous depth")
    launch("dvmvs_depth_reproject_lowres_fwd", previous_depth.device, ptr(transformation.contiguous()), ptr(previous_depth.contiguous()),
           ptr(full_K.contiguous()), ptr(half_K.contiguous()), ptr(zbuffer), ptr(out_lowres), int(factor), B, Hf, Wf)
    return out_lowres


def depth_reproject_estimate_into(transformation: Tensor, previous_depth: Tensor, full_K: Tensor, half_K: Tensor, estimate: Tensor,
                                  estimate_to_clear: Optional[Tensor], factor: int) -> Tensor:
    """The frame path's re-projection in one launch (dvmvs_depth_reproject_estimate_fwd): splat straight into ``estimate``
    [B,1,H/2/f,W/2/f] (all-zero on entry), zero-filling ``estimate_to_clear`` (the buffer of the frame after next) on the way."""
    check_tensors("depth_reproject_estimate_into", transformation, previous_depth, full_K, half_K, estimate)
    B, one, Hf, Wf = previous_depth.shape
    shape = (B, 1, Hf // 2 // factor, Wf // 2 // factor)
    if one != 1 or tuple(estimate.shape) != shape or not estimate.is_contiguous() or not previous_depth.is_contiguous() or \
            (estimate_to_clear is not None and (tuple(estimate_to_clear.shape) != shape or not estimate_to_clear.is_contiguous() or
                                                estimate_to_clear.data_ptr() == estimate.data_ptr())):
        raise ValueError("dvmvs::depth_reproject_estimate_into: expected contiguous [B,1,H,W] depth and distinct [B,1,H/2/f,W/2/f] estimate buffers")
    launch("dvmvs_depth_reproject_estimate_fwd", previous_depth.device, ptr(transformation.contiguous()), ptr(previous_depth),
           ptr(full_K.contiguous()), ptr(half_K.contiguous()), ptr(estimate), opt_ptr(estimate_to_clear), int(factor), B, Hf, Wf)
    return estimate


# ----------------------------------------------------------------------------------------------------------------------
# frame-path epilogues, up-sampling and depthwise convolutions as registered ops (autograd: up-sampling and depthwise_conv_train only)
# ----------------------------------------------------------------------------------------------------------------------
def _residual_shape(residual_mode, B, C, H, W):
    return (B, C, H, W) if residual_mode == RESIDUAL_SAME else (B, C, H // 2, W // 2)


@custom_op("bias_act_", mutates_args=("x",))
def bias_act_(x: Tensor, bias: Tensor, activation: int, residual: Tensor, residual_mode: int) -> None:
    """In place: x[b,c] = act(x[b,c] + bias[c]) (+ residual) for a contiguous NCHW tensor.  ``bias`` / ``residual`` may be
    empty (numel 0); residual_mode 1: same shape, 2: half resolution, nearest-up-sampled on the fly."""
    check_tensors("bias_act_", x)
    if not x.is_contiguous() or x.dim() != 4:
        raise ValueError("dvmvs::bias_act_: expected a contiguous NCHW tensor")
    B, C, H, W = x.shape
    bias = bias.contiguous()
    bias_ptr, res_ptr = channel_ptr("bias_act_", "bias", bias, C), None
    if residual_mode != RESIDUAL_NONE:
        want = _residual_shape(residual_mode, B, C, H, W)
        if tuple(residual.shape) != want:
            raise ValueError(f"dvmvs::bias_act_: residual {tuple(residual.shape)} does not match {want}")
        residual = residual.contiguous()
        res_ptr = ptr(residual)
    launch("dvmvs_bias_act_inplace", x.device, ptr(x), bias_ptr, res_ptr, int(residual_mode), B, C, H, W, int(activation))


def _upsample2x_fake(x):
    B, C, H, W = x.shape
    return x.new_empty((B, C, 2 * H, 2 * W))


@custom_op("upsample2x", fake=_upsample2x_fake)
def upsample2x(x: Tensor) -> Tensor:
    check_tensors("upsample2x", x)
    x = x.contiguous()
    B, C, H, W = x.shape
    out = torch.empty((B, C, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
    launch("dvmvs_upsample2x_fwd", x.device, ptr(x), ptr(out), 0, None, 0, B, C, H, W)
    return out


def _upsample2x_bwd_fake(grad_out):
    B, C, OH, OW = grad_out.shape
    return grad_out.new_empty((B, C, OH // 2, OW // 2))


@custom_op("upsample2x_bwd", fake=_upsample2x_bwd_fake)
def upsample2x_bwd(grad_out: Tensor) -> Tensor:
    """Adjoint of ``upsample2x`` as a gather (no atomics: bit-reproducible), dvmvs_upsample2x_bwd."""
    check_tensors("upsample2x_bwd", grad_out)
    grad_out = grad_out.contiguous()
    B, C, OH, OW = grad_out.shape
    grad_in = torch.empty((B, C, OH // 2, OW // 2), dtype=torch.float32, device=grad_out.device)
    launch("dvmvs_upsample2x_bwd", grad_out.device, ptr(grad_out), ptr(grad_in), B, C, OH // 2, OW // 2)
    return grad_in


torch.library.register_autograd("dvmvs::upsample2x", lambda ctx, grad: upsample2x_bwd(grad), setup_context=lambda ctx, inputs, output: None)


def _depthwise_out_shape(name, x, weight, stride):
    """[B,C,OH,OW] of a depthwise k x k convolution (weight [C,1,k,k], padding k//2) of ``x``."""
    B, C, H, W = x.shape
    k = weight.shape[-1]
    if tuple(weight.shape) != (C, 1, k, k):
        raise ValueError(f"dvmvs::{name}: weight {tuple(weight.shape)} is not depthwise for {C} channels")
    pad = k // 2
    return B, C, (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


@custom_op("depthwise_conv_train", fake=lambda x, weight, stride: x.new_empty(_depthwise_out_shape("depthwise_conv_train", x, weight, stride)))
def depthwise_conv_train(x: Tensor, weight: Tensor, stride: int) -> Tensor:
    """Depthwise k x k convolution (weight [C,1,k,k], padding k//2, no bias) with gradients: the training-time form of
    ``depthwise_conv`` (MIOpen runs these MnasNet layers, forward and backward, through its naive reference kernels)."""
    check_tensors("depthwise_conv_train", x, weight)
    x, weight = x.contiguous(), weight.contiguous()
    B, C, H, W = x.shape
    out = torch.empty(_depthwise_out_shape("depthwise_conv_train", x, weight, stride), dtype=torch.float32, device=x.device)
    launch("dvmvs_depthwise_conv_fwd", x.device, ptr(x), ptr(weight), None, None, 0, ptr(out), B, C, H, W, weight.shape[-1], int(stride), 0)
    return out


def _depthwise_bwd_fake(grad_out, x, weight, stride, need_input, need_weight):
    return (torch.empty_like(x) if need_input else x.new_empty(0)), (torch.empty_like(weight) if need_weight else x.new_empty(0))


@custom_op("depthwise_conv_bwd", fake=_depthwise_bwd_fake)
def depthwise_conv_bwd(grad_out: Tensor, x: Tensor, weight: Tensor, stride: int, need_input: bool, need_weight: bool) -> Tuple[Tensor, Tensor]:
    """(grad_x, grad_weight) of ``depthwise_conv_train`` (gathers / a fixed-order reduction: no atomics); an unneeded one is empty."""
    check_tensors("depthwise_conv_bwd", grad_out, x, weight)
    grad_out, x, weight = grad_out.contiguous(), x.contiguous(), weight.contiguous()
    B, C, H, W = x.shape
    k = weight.shape[-1]
    gx = torch.empty_like(x) if need_input else x.new_empty(0)
    gw = torch.empty_like(weight) if need_weight else x.new_empty(0)
    scratch = _capi.lib().dvmvs_depthwise_conv_bwd_workspace_bytes(B, C, H, W, k, int(stride)) if need_weight else 0
    workspace = torch.empty(scratch // 4, dtype=torch.float32, device=x.device) if scratch else None
    launch("dvmvs_depthwise_conv_bwd", x.device, ptr(grad_out), ptr(x), ptr(weight), ptr(gx) if need_input else None,
           ptr(gw) if need_weight else None, opt_ptr(workspace), B, C, H, W, k, int(stride))
    return gx, gw


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


def _depthwise_fake(x, weight, bias, stride, activation, pre_bias, pre_relu):
    return x.new_empty(_depthwise_out_shape("depthwise_conv", x, weight, stride))


@custom_op("depthwise_conv", fake=_depthwise_fake)
def depthwise_conv(x: Tensor, weight: Tensor, bias: Tensor, stride: int, activation: int, pre_bias: Tensor, pre_relu: bool) -> Tensor:
    """Depthwise k x k convolution (weight [C,1,k,k], padding k//2) + bias (numel 0 = none) + activation, one HIP launch.  With
    ``pre_relu`` the input is the raw output of the preceding 1x1 convolution and relu(x + pre_bias[c]) (numel 0 = no bias) is applied
    to it on the fly."""
    check_tensors("depthwise_conv", x, weight)
    x, weight, bias, pre_bias = x.contiguous(), weight.contiguous(), bias.contiguous(), pre_bias.contiguous()
    B, C, H, W = x.shape
    out = torch.empty(_depthwise_out_shape("depthwise_conv", x, weight, stride), dtype=torch.float32, device=x.device)
    launch("dvmvs_depthwise_conv_fwd", x.device, ptr(x), ptr(weight), channel_ptr("depthwise_conv", "bias", bias, C),
           channel_ptr("depthwise_conv", "pre_bias", pre_bias, C), int(bool(pre_relu)), ptr(out), B, C, H, W, weight.shape[-1], int(stride),
           int(activation))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# destination-passing forms for the frame engine (inference, no autograd, hipGraph-capturable): the producer writes straight
# into a channel slice of a concatenation buffer or into a state buffer, so that torch.cat / copy_ launches disappear from
# the frame.  Plain functions over the C ABI, not torch.library ops: nothing here allocates or needs shape inference.
# ----------------------------------------------------------------------------------------------------------------------
def _slice_batch_stride(name, dst, B, C, H, W):
    """``dst`` must be [B,C,H,W] with dense planes and channels (a channel slice of a contiguous NCHW buffer); returns its batch
    stride in elements."""
    check_tensors(name, dst)
    if tuple(dst.shape) != (B, C, H, W) or dst.stride(3) != 1 or dst.stride(2) != W or dst.stride(1) != H * W:
        raise ValueError(f"dvmvs::{name}: buffer {tuple(dst.shape)} / strides {dst.stride()} is not a channel slice of a "
                         f"contiguous NCHW buffer for [{B},{C},{H},{W}]")
    return dst.stride(0) if B > 1 else C * H * W


def bias_act_into(x: Tensor, dst: Tensor, bias, activation: int, residual=None, residual_mode: int = RESIDUAL_NONE, p0: float = 0.0,
                  p1: float = 0.0) -> Tensor:
    """dst = act(x + bias[c]) (+ residual); ``x`` a dense convolution output, ``dst`` x itself or a channel slice (see above)."""
    check_tensors("bias_act_into", x)
    if not x.is_contiguous() or x.dim() != 4:
        raise ValueError("dvmvs::bias_act_into: expected a contiguous NCHW source")
    B, C, H, W = x.shape
    stride = _slice_batch_stride("bias_act_into", dst, B, C, H, W)
    bias_ptr, res_ptr = channel_ptr("bias_act_into", "bias", bias, C), None
    if residual_mode != RESIDUAL_NONE:
        want = _residual_shape(residual_mode, B, C, H, W)
        if tuple(residual.shape) != want or not residual.is_contiguous():
            raise ValueError(f"dvmvs::bias_act_into: residual {tuple(residual.shape)} does not match {want} (contiguous)")
        res_ptr = ptr(residual)
    launch("dvmvs_bias_act_fwd", x.device, ptr(x), ptr(dst), stride, bias_ptr, res_ptr, int(residual_mode), B, C, H, W, int(activation),
           float(p0), float(p1))
    return dst


def conv_bias_act_into(x: Tensor, weight: Tensor, bias: Tensor, dst, stride: int, padding: int, activation: int):
    """conv2d(x, weight, padding, stride) + bias [+ ReLU] as ONE MIOpen fusion plan (dvmvs_conv_bias_act_fwd), written into ``dst``
    (a dense tensor or a channel slice of a concatenation buffer; None: a new tensor).  Returns the output, or None when MIOpen has
    no fused plan for the problem (the caller then runs convolution + dvmvs_bias_act_fwd)."""
    check_tensors("conv_bias_act_into", x, weight, bias)
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
    with torch.cuda.device(x.device):     # not ``launch``: EUNSUPPORTED is an answer here, not an error
        rc = _capi.lib().dvmvs_conv_bias_act_fwd(ptr(x), ptr(weight), ptr(bias), ptr(dst), batch_stride, B, Cin, H, W, Cout, K,
                                                 int(stride), int(padding), int(activation), torch.cuda.current_stream(x.device).cuda_stream)
    if rc == EUNSUPPORTED:
        return None
    _capi.check(rc, "dvmvs_conv_bias_act_fwd")
    return dst


def upsample2x_into(x: Tensor, dst: Tensor, pre_bias=None, pre_activation: int = 0) -> Tensor:
    """x2 bilinear (align_corners) up-sampling of ``x`` into ``dst``; with ``pre_activation`` (ACTIVATIONS) ``x`` is a raw convolution
    output and act(x + pre_bias[c]) is applied to the taps on the fly."""
    check_tensors("upsample2x_into", x)
    x = x.contiguous()
    B, C, H, W = x.shape
    stride = _slice_batch_stride("upsample2x_into", dst, B, C, 2 * H, 2 * W)
    launch("dvmvs_upsample2x_fwd", x.device, ptr(x), ptr(dst), stride, channel_ptr("upsample2x_into", "pre_bias", pre_bias, C),
           int(pre_activation), B, C, H, W)
    return dst


def upsample2x_pair_into(x1: Tensor, dst1: Tensor, x2: Tensor, dst2: Tensor, pre_bias2=None, pre_activation2: int = 0) -> None:
    """``upsample2x_into(x1, dst1)`` and ``upsample2x_into(x2, dst2, pre_bias2, pre_activation2)`` for two maps of the same size in ONE launch
    (dvmvs_upsample2x_pair_fwd: a decoder level's feature map and its depth head); the same values bit for bit."""
    check_tensors("upsample2x_pair_into", x1, x2)
    x1, x2 = x1.contiguous(), x2.contiguous()
    B, C1, H, W = x1.shape
    C2 = x2.shape[1]
    if tuple(x2.shape) != (B, C2, H, W):
        raise ValueError(f"dvmvs::upsample2x_pair_into: the two maps must have the same batch and size, got {tuple(x1.shape)} and {tuple(x2.shape)}")
    stride1 = _slice_batch_stride("upsample2x_pair_into", dst1, B, C1, 2 * H, 2 * W)
    stride2 = _slice_batch_stride("upsample2x_pair_into", dst2, B, C2, 2 * H, 2 * W)
    launch("dvmvs_upsample2x_pair_fwd", x1.device, ptr(x1), ptr(dst1), stride1, C1, ptr(x2), ptr(dst2), stride2,
           channel_ptr("upsample2x_pair_into", "pre_bias2", pre_bias2, C2), int(pre_activation2), C2, B, H, W)


# ---- 3x3 convolutions on the bottleneck maps (csrc/bottleneck_conv.hip): weight-streaming fp32 MFMA GEMM, deterministic split-K ----
def bottleneck_conv_splits(B: int, C_out: int, C_in: int, H_in: int, W_in: int, stride: int) -> int:
    """Number of K-splits (partial sums) dvmvs_bottleneck_conv_fwd produces for this problem; 0 when the kernel does not take it
    (other map sizes, C_in not a multiple of 16): the caller stays on MIOpen."""
    n = _capi.lib().dvmvs_bottleneck_conv_splits(int(B), int(C_out), int(C_in), int(H_in), int(W_in), int(stride))
    return n if n > 0 else 0


def _packed_weights(entry, weight, nbytes, *args):
    """The float32 buffer of ``nbytes`` that the C entry ``entry`` packs ``weight`` into."""
    packed = torch.empty(nbytes // 4, dtype=torch.float32, device=weight.device)
    launch(entry, weight.device, ptr(weight.contiguous()), ptr(packed), *args)
    return packed


def bottleneck_conv_pack(weight: Tensor) -> Tensor:
    """[C_out, C_in, 3, 3] convolution weights re-packed once into the MFMA A-operand order the kernel streams."""
    check_tensors("bottleneck_conv_pack", weight)
    C_out, C_in, kh, kw = weight.shape
    nbytes = _capi.lib().dvmvs_bottleneck_conv_packed_bytes(C_out, C_in) if (kh, kw) == (3, 3) else 0
    if nbytes == 0:
        raise ValueError(f"dvmvs::bottleneck_conv_pack: need a 3x3 kernel and C_in % 16 == 0, got {tuple(weight.shape)}")
    return _packed_weights("dvmvs_bottleneck_conv_pack", weight, nbytes, C_out, C_in)


def bottleneck_conv_into(x: Tensor, packed: Tensor, C_out: int, stride: int, partials: Tensor, upsample: bool = False) -> int:
    """3x3, padding 1 convolution of ``x`` [B,C_in,H,W] with ``bottleneck_conv_pack``-ed weights as K-split partial sums into
    ``partials`` (at least splits * B * C_out * H_out * W_out floats, laid out [split][B][C_out][H_out*W_out]).  Returns the number of
    splits; the consumer adds them in ascending order (``partial_sums_bias_act_into`` / ``lstm_gates_partials_into``).
    ``upsample``: the layer convolves the 2x bilinear up-sampling (align_corners=True, ``upsample2x``'s values bit for bit) of ``x``
    [B,C_in,H/2,W/2], interpolated while the input is staged (dvmvs_bottleneck_conv_up2x_fwd: the 16x20 map, stride 1)."""
    check_tensors("bottleneck_conv_into", x, packed, partials)
    B, C_in, H, W = x.shape
    if upsample:
        H, W = 2 * H, 2 * W
    splits = bottleneck_conv_splits(B, C_out, C_in, H, W, stride) if not upsample or (H, W, stride) == (16, 20, 1) else 0
    if splits == 0:
        raise ValueError(f"dvmvs::bottleneck_conv_into: problem {tuple(x.shape)} -> {C_out} (stride {stride}{', up-sampled' if upsample else ''}) "
                         f"is not one of the bottleneck shapes")
    if not x.is_contiguous() or partials.numel() < splits * B * C_out * (H // stride) * (W // stride) or not partials.is_contiguous():
        raise ValueError("dvmvs::bottleneck_conv_into: expected a contiguous input and a partial-sum buffer of splits * B * C_out * H_out * W_out floats")
    if upsample:
        launch("dvmvs_bottleneck_conv_up2x_fwd", x.device, ptr(x), ptr(packed), ptr(partials), B, C_in, H, W, int(C_out))
    else:
        launch("dvmvs_bottleneck_conv_fwd", x.device, ptr(x), ptr(packed), ptr(partials), B, C_in, H, W, int(C_out), int(stride))
    return splits


def partial_sums_bias_act_into(partials: Tensor, n_partials: int, dst: Tensor, bias, activation: int, shape) -> Tensor:
    """dst = act(sum of the partial sums + bias[c]); ``dst`` a dense [B,C,H,W] tensor or a channel slice of a concatenation buffer."""
    check_tensors("partial_sums_bias_act_into", partials)
    B, C, H, W = shape
    stride = _slice_batch_stride("partial_sums_bias_act_into", dst, B, C, H, W)
    launch("dvmvs_partial_sums_bias_act_fwd", dst.device, ptr(partials), int(n_partials), ptr(dst), stride,
           channel_ptr("partial_sums_bias_act_into", "bias", bias, C), B, C, H * W, int(activation))
    return dst


# ---- dense 3x3 / 5x5 convolutions of the larger maps (csrc/direct_conv.hip): direct fp32 MFMA convolution, bias + ReLU fused ----
def direct_conv_tile(B: int, C_in: int, H: int, W: int, C_out: int, kernel_size: int, stride: int) -> int:
    """0 when dvmvs_direct_conv_fwd does not take the problem (the caller keeps its library convolution); else the number of
    16-channel output tiles per wave (1 or 2) to pack the weights for."""
    return _capi.lib().dvmvs_direct_conv_tile(int(B), int(C_in), int(H), int(W), int(C_out), int(kernel_size), int(stride))


def direct_conv_shape(B: int, C_in: int, H: int, W: int, C_out: int, kernel_size: int, stride: int) -> int:
    """0 when dvmvs_direct_conv_fwd does not take the problem; else the id (1..4) of the workgroup shape it runs with, which together with
    the kernel size and the stride names the compiled kernel (ids 1 and 2 pack for ``direct_conv_tile`` 2, ids 3 and 4 for 1)."""
    return _capi.lib().dvmvs_direct_conv_shape(int(B), int(C_in), int(H), int(W), int(C_out), int(kernel_size), int(stride))


def direct_conv_pack(weight: Tensor, n_tile: int) -> Tensor:
    """[C_out, C_in, k, k] convolution weights re-packed once into the MFMA B-operand order the kernel streams."""
    check_tensors("direct_conv_pack", weight)
    C_out, C_in, kh, kw = weight.shape
    nbytes = _capi.lib().dvmvs_direct_conv_packed_bytes(C_out, C_in, kh, int(n_tile)) if kh == kw else 0
    if nbytes == 0:
        raise ValueError(f"dvmvs::direct_conv_pack: need a 3x3 or 5x5 kernel and C_out % (16 * n_tile) == 0, got {tuple(weight.shape)}, n_tile {n_tile}")
    return _packed_weights("dvmvs_direct_conv_pack", weight, nbytes, C_out, C_in, kh, int(n_tile))


def direct_conv_into(x: Tensor, packed: Tensor, n_tile: int, bias, dst: Tensor, C_out: int, kernel_size: int, stride: int, activation: int,
                     dst_nhwc=None) -> Tensor:
    """dst = act(conv2d(x, W, padding = k // 2, stride) + bias) with ``direct_conv_pack``-ed weights; ``dst`` a dense [B,C_out,H/s,W/s]
    tensor or a channel slice of a concatenation buffer; activation "none" or "relu".  ``dst_nhwc``: a second destination that receives the
    same values channels-last ([B,C_out,H/s,W/s] in torch.channels_last memory format), written in the same epilogue."""
    check_tensors("direct_conv_into", x, packed)
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError("dvmvs::direct_conv_into: expected a contiguous NCHW input")
    B, C_in, H, W = x.shape
    C_out = int(C_out)
    batch_stride = _slice_batch_stride("direct_conv_into", dst, B, C_out, H // stride, W // stride)
    if dst_nhwc is not None:
        check_tensors("direct_conv_into", dst_nhwc)
        if tuple(dst_nhwc.shape) != (B, C_out, H // stride, W // stride) or not dst_nhwc.is_contiguous(memory_format=torch.channels_last):
            raise ValueError("dvmvs::direct_conv_into: dst_nhwc must be a dense channels-last tensor of the output's shape")
    launch("dvmvs_direct_conv_dual_fwd", x.device, ptr(x), 0, ptr(packed), int(n_tile), channel_ptr("direct_conv_into", "bias", bias, C_out),
           ptr(dst), batch_stride, opt_ptr(dst_nhwc), B, C_in, H, W, C_out, int(kernel_size), int(stride), int(activation))
    return dst


# ---- 1x1 convolutions (csrc/pointwise_conv.hip): fp32 MFMA GEMM from the NCHW map, bias + ReLU + residual in its store path ----
def pointwise_conv_supported(B: int, C_in: int, H: int, W: int, C_out: int, activation: int, residual_mode: int) -> bool:
    """Whether dvmvs_pointwise_conv_fwd takes the problem (else the caller keeps its library convolution + epilogue launch)."""
    return bool(_capi.lib().dvmvs_pointwise_conv_supported(int(B), int(C_in), int(H), int(W), int(C_out), int(activation), int(residual_mode)))


def pointwise_conv_pack(weight: Tensor) -> Tensor:
    """[C_out,C_in,1,1] (or [C_out,C_in]) -> the kernel's B-operand order; once per layer (the weights are constants at inference)."""
    check_tensors("pointwise_conv_pack", weight)
    if weight.dim() not in (2, 4) or (weight.dim() == 4 and tuple(weight.shape[2:]) != (1, 1)):
        raise ValueError(f"dvmvs::pointwise_conv_pack: need a [C_out,C_in,1,1] weight, got {tuple(weight.shape)}")
    C_out, C_in = int(weight.shape[0]), int(weight.shape[1])
    return _packed_weights("dvmvs_pointwise_conv_pack", weight, _capi.lib().dvmvs_pointwise_conv_packed_bytes(C_out, C_in), C_out, C_in)


def pointwise_conv_into(x: Tensor, packed: Tensor, bias, dst: Tensor, C_out: int, activation: int, residual=None, residual_mode: int = 0,
                        splits: int = 0) -> Tensor:
    """dst = act(conv1x1(x, W) + bias) + residual with ``pointwise_conv_pack``-ed weights; ``dst`` a dense [B,C_out,H,W] tensor or a channel
    slice of a concatenation buffer; activation "none" or "relu"; ``residual`` / ``residual_mode`` as ``bias_act_into`` (1: same shape,
    2: half resolution, nearest-up-sampled)."""
    check_tensors("pointwise_conv_into", x, packed)
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError("dvmvs::pointwise_conv_into: expected a contiguous NCHW input")
    B, C_in, H, W = x.shape
    C_out = int(C_out)
    if packed.numel() * 4 != _capi.lib().dvmvs_pointwise_conv_packed_bytes(C_out, C_in):
        raise ValueError(f"dvmvs::pointwise_conv_into: the packed weights are not those of a {C_in} -> {C_out} layer")
    batch_stride = _slice_batch_stride("pointwise_conv_into", dst, B, C_out, H, W)
    bias_ptr, res_ptr, residual_stride = channel_ptr("pointwise_conv_into", "bias", bias, C_out), None, 0
    if residual_mode:
        residual_stride = _slice_batch_stride("pointwise_conv_into", residual, *_residual_shape(residual_mode, B, C_out, H, W))
        res_ptr = ptr(residual)
    launch("dvmvs_pointwise_conv_fwd", x.device, ptr(x), 0, ptr(packed), bias_ptr, res_ptr, residual_stride, int(residual_mode), ptr(dst),
           batch_stride, B, C_in, H, W, C_out, int(activation), int(splits))
    return dst


def conv_head_into(x: Tensor, weight: Tensor, bias, dst: Tensor, activation: int = 0, p0: float = 0.0, p1: float = 0.0) -> Tensor:
    """3x3, padding 1 convolution with ONE output channel (the decoder's depth heads): dst [B,1,H,W] = act(conv(x, weight) + bias);
    bias None and activation 0: the raw convolution output (the consumer applies bias + activation)."""
    check_tensors("conv_head_into", x, weight)
    if x.dim() != 4 or not x.is_contiguous() or tuple(weight.shape) != (1, x.shape[1], 3, 3) or not weight.is_contiguous():
        raise ValueError(f"dvmvs::conv_head_into: expected a contiguous NCHW input and a [1,{x.shape[1]},3,3] weight, got {tuple(x.shape)}, {tuple(weight.shape)}")
    B, C_in, H, W = x.shape
    batch_stride = _slice_batch_stride("conv_head_into", dst, B, 1, H, W)
    launch("dvmvs_conv_head_fwd", x.device, ptr(x), 0, ptr(weight), channel_ptr("conv_head_into", "bias", bias, 1), ptr(dst), batch_stride,
           B, C_in, H, W, int(activation), float(p0), float(p1))
    return dst


# ---- several small device-to-device copies in one launch ----
def copy_batch(pairs) -> None:
    """``dst.copy_(src)`` for up to eight (dst, src) pairs of equally laid out dense float32 device tensors in ONE launch (dvmvs_copy_batch).
    The caller guarantees what the C entry requires: same shape and strides per pair, dense storage, 16-byte aligned, a multiple of 4
    elements, no overlap between pairs (``batchable`` checks one pair)."""
    n = len(pairs)
    srcs, dsts, counts = (ctypes.c_void_p * n)(), (ctypes.c_void_p * n)(), (ctypes.c_longlong * n)()
    for j, (dst, src) in enumerate(pairs):
        srcs[j], dsts[j], counts[j] = src.data_ptr(), dst.data_ptr(), dst.numel()
    launch("dvmvs_copy_batch", pairs[0][0].device, srcs, dsts, counts, n)


def batchable(dst: Tensor, src: Tensor) -> bool:
    """Whether ``dst.copy_(src)`` is a flat copy dvmvs_copy_batch can take."""
    return (dst.is_cuda and src.is_cuda and dst.device == src.device and dst.dtype == torch.float32 and src.dtype == torch.float32
            and dst.shape == src.shape and dst.numel() % 4 == 0 and dst.numel() > 0 and dst.data_ptr() % 16 == 0 and src.data_ptr() % 16 == 0
            and ((dst.is_contiguous() and src.is_contiguous())
                 or (dst.dim() == 4 and dst.is_contiguous(memory_format=torch.channels_last) and src.is_contiguous(memory_format=torch.channels_last))))

"""The ops of the baselines (inference only): the RGB SAD sweep into the encoder input of MVDepthNet and GP-MVS, GP-MVS's filter step,
and DPSNet's plane volume and up-sampling soft-argmin."""
from typing import Sequence, Tuple

import torch
from torch import Tensor

from dvmvs.hip import _capi
from dvmvs.hip.ops._common import check_tensors, custom_op, launch, ptr
from dvmvs.hip.ops.sweep import _check_sweep_matrices


@custom_op("rgb_sweep", mutates_args=("out",), fake=lambda *args: None)
def rgb_sweep(out: Tensor, image1: Tensor, image2s: Sequence[Tensor], Hm: Tensor, kt: Tensor, min_depth: float, max_depth: float,
              n_depth_levels: int, channel_offset: int, copy_image: bool) -> None:
    """In place: ``out[:, channel_offset:channel_offset + n_depth_levels]`` = the SAD cost volume of the 3-channel ``image1`` against
    ``image2s`` (cost_volume_fusion(..., dot_product=False)); with ``copy_image`` also ``out[:, 0:3] = image1``.  ``out`` is a
    contiguous [B,Cout,H,W] tensor; no other channel is written.  Bit-identical to ``cost_volume(..., dot_product=False, variant=1)``."""
    check_tensors("rgb_sweep", out, image1, Hm, kt, *image2s)
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
    launch("dvmvs_rgb_sweep_fwd", out.device, ptr(image1), _capi.pointer_array([ptr(t) for t in image2s]), ptr(Hm.contiguous()),
           ptr(kt.contiguous()), ptr(out), B, M, C, H, W, int(n_depth_levels), float(min_depth), float(max_depth), out.shape[1],
           int(channel_offset), int(bool(copy_image)))


@custom_op("gp_filter_step", mutates_args=("state",), fake=lambda state, y, A, k, reset: torch.empty_like(y))
def gp_filter_step(state: Tensor, y: Tensor, A: Sequence[float], k: Sequence[float], reset: bool) -> Tensor:
    """One step of GP-MVS's Kalman filter: ``state`` [2,N] float64 in place (M <- A M; M <- M + k (y - M[0])), returns
    relu(float32(M[0])) shaped like ``y`` (fp32, N elements).  ``A`` = the 2x2 transition row-major, ``k`` the gain (host
    algebra: dvmvs.baselines.runner.GPFilter); ``reset`` starts from M = 0."""
    check_tensors("gp_filter_step", y)
    check_tensors("gp_filter_step", state, dtype=torch.float64, label="state", shape=(2, y.numel()), device=y.device, contiguous=True)
    if len(A) != 4 or len(k) != 2:
        raise ValueError("dvmvs::gp_filter_step: A has 4 entries (row-major 2x2), k has 2")
    y = y.contiguous()
    z = torch.empty_like(y)
    launch("dvmvs_gp_filter_step", y.device, ptr(state), ptr(y), ptr(z), y.numel(), float(A[0]), float(A[1]), float(A[2]), float(A[3]),
           float(k[0]), float(k[1]), int(bool(reset)))
    return z


def _dps_volume_fake(ref, meas, pose, K, Kinv, nlabel, mindepth):
    B, C, h, w = ref.shape
    return ref.new_empty((B, 2 * C, nlabel, h, w))


@custom_op("dps_volume", fake=_dps_volume_fake)
def dps_volume(ref: Tensor, meas: Tensor, pose: Tensor, K: Tensor, Kinv: Tensor, nlabel: int, mindepth: float) -> Tensor:
    """[B,2C,nlabel,h,w]: channels 0..C-1 = ``ref`` at every plane, channels C..2C-1 = ``meas`` warped to plane i at depth
    mindepth * nlabel / (i + 1e-16) with DPSNet's ``inverse_warp`` (K^-1 un-projection, Z >= 1e-3, (w - 1) normalisation, coordinates
    outside [-1, 1] fully masked).  ``pose`` [B,3,4] maps the reference camera to the measurement camera; ``K`` / ``Kinv`` [B,3,3] are
    the intrinsics at the resolution of the features."""
    check_tensors("dps_volume", ref, meas, pose, K, Kinv)
    if ref.dim() != 4 or meas.shape != ref.shape:
        raise ValueError(f"dvmvs::dps_volume: expected two [B,C,h,w] feature maps, got {tuple(ref.shape)} and {tuple(meas.shape)}")
    B, C, h, w = ref.shape
    if tuple(pose.shape) != (B, 3, 4) or tuple(K.shape) != (B, 3, 3) or tuple(Kinv.shape) != (B, 3, 3):
        raise ValueError(f"dvmvs::dps_volume: expected pose [{B},3,4] and K, Kinv [{B},3,3], got {tuple(pose.shape)}, {tuple(K.shape)}, "
                         f"{tuple(Kinv.shape)}")
    ref, meas, pose, K, Kinv = (t.contiguous() for t in (ref, meas, pose, K, Kinv))
    out = torch.empty((B, 2 * C, int(nlabel), h, w), dtype=torch.float32, device=ref.device)
    launch("dvmvs_dps_volume_fwd", ref.device, ptr(ref), ptr(meas), ptr(pose), ptr(K), ptr(Kinv), ptr(out), B, C, h, w, int(nlabel),
           float(mindepth))
    return out


def _dps_regress_fake(costs, height, width, mindepth, with_pred=True):
    B = costs.shape[0]
    return costs.new_empty((B, 1, height, width)), costs.new_empty((B, height, width) if with_pred else (0,))


@custom_op("dps_regress", fake=_dps_regress_fake)
def dps_regress(costs: Tensor, height: int, width: int, mindepth: float, with_pred: bool = True) -> Tuple[Tensor, Tensor]:
    """(depth [B,1,H,W], pred [B,H,W]) of DPSNet's regression: the plane costs [B,nlabel,h,w] or [B,1,nlabel,h,w] are up-sampled to
    (``height``, ``width``) per plane (bilinear, half-pixel centres), then pred = sum_i softmax_i * i and
    depth = mindepth * nlabel / (pred + 1e-16).  With ``with_pred`` False the expectation is not written (an empty tensor is returned)."""
    check_tensors("dps_regress", costs)
    if costs.dim() == 5 and costs.shape[1] == 1:
        costs = costs[:, 0]
    if costs.dim() != 4:
        raise ValueError(f"dvmvs::dps_regress: expected costs [B,nlabel,h,w] or [B,1,nlabel,h,w], got {tuple(costs.shape)}")
    costs = costs.contiguous()
    B, nlabel, h, w = costs.shape
    H, W = int(height), int(width)
    depth = torch.empty((B, 1, H, W), dtype=torch.float32, device=costs.device)
    pred = torch.empty((B, H, W) if with_pred else (0,), dtype=torch.float32, device=costs.device)
    launch("dvmvs_dps_regress_fwd", costs.device, ptr(costs), ptr(depth), ptr(pred) if with_pred else None, B, nlabel, h, w, H, W,
           float(mindepth))
    return depth, pred

"""DPSNet (the reference's dvmvs/baselines/dpsnet/dpsnet.py) at the same import path, with the same parameter names and shapes.

``PSNet.forward`` has two routes:

* fused (CUDA tensors, no input requiring grad): the plane volume of a measurement frame is one dvmvs::dps_volume launch
  (csrc/dps_volume.hip) instead of nlabel inverse_warp calls and 2 nlabel slice copies; the context network runs once on all planes as
  a batch of nlabel instead of nlabel batch-1 calls; up-sampling, softmax and expectation are one dvmvs::dps_regress launch
  (csrc/dps_regress.hip) for each of the two outputs.  The feature extractor and the 3-D convolutions are torch.nn modules on MIOpen.
  There is no fallback: without the HIP library this route raises.
* plain (CPU tensors, or any input requiring grad: tests and training): torch operations in the reference's order.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from dvmvs.utils import freeze_batchnorm


# ----------------------------------------------------------------------------------------------------------------------
# DPSNet's warp (not the convention of dvmvs.utils: K^-1 un-projection, Z >= 1e-3, (w - 1) normalisation, mask to 2)
# ----------------------------------------------------------------------------------------------------------------------
def pixel_grid(height, width, like):
    """[1,3,H*W] homogeneous pixel coordinates (x, y, 1) in the dtype and on the device of ``like``."""
    ys = torch.arange(0, height, device=like.device).view(height, 1).expand(height, width)
    xs = torch.arange(0, width, device=like.device).view(1, width).expand(height, width)
    return torch.stack((xs, ys, torch.ones_like(xs)), dim=0).to(like.dtype).reshape(1, 3, height * width)


def pixel2cam(depth, intrinsics_inv):
    """Camera-frame points [B,3,H,W] of a depth map [B,H,W]."""
    b, h, w = depth.shape
    rays = intrinsics_inv.bmm(pixel_grid(h, w, depth).expand(b, 3, h * w).contiguous()).view(b, 3, h, w)
    return rays * depth.unsqueeze(1)


def cam2pixel(cam_coords, proj_c2p_rot, proj_c2p_tr, padding_mode):
    """Normalised [-1,1] sample positions [B,H,W,2] of camera-frame points [B,3,H,W]; with 'zeros' padding, a coordinate outside
    [-1,1] is set to 2 so that the sample reads no image content at all."""
    b, _, h, w = cam_coords.shape
    p = cam_coords.reshape(b, 3, -1)
    if proj_c2p_rot is not None:
        p = proj_c2p_rot.bmm(p)
    if proj_c2p_tr is not None:
        p = p + proj_c2p_tr
    X, Y = p[:, 0], p[:, 1]
    Z = p[:, 2].clamp(min=1e-3)
    X_norm = 2 * (X / Z) / (w - 1) - 1
    Y_norm = 2 * (Y / Z) / (h - 1) - 1
    if padding_mode == "zeros":
        X_norm = torch.where((X_norm > 1) | (X_norm < -1), torch.full_like(X_norm, 2), X_norm)
        Y_norm = torch.where((Y_norm > 1) | (Y_norm < -1), torch.full_like(Y_norm, 2), Y_norm)
    return torch.stack([X_norm, Y_norm], dim=2).view(b, h, w, 2)


def inverse_warp(feat, depth, pose, intrinsics, intrinsics_inv, padding_mode="zeros"):
    """``feat`` [B,C,H,W] of the source view sampled where the target view's pixels at ``depth`` [B,H,W] project to; ``pose`` [B,3,4]
    maps the target camera to the source camera."""
    if depth.dim() != 3 or tuple(pose.shape[1:]) != (3, 4) or tuple(intrinsics.shape[1:]) != (3, 3) or intrinsics_inv.shape != intrinsics.shape:
        raise ValueError(f"inverse_warp: expected depth [B,H,W], pose [B,3,4], intrinsics [B,3,3]; got {tuple(depth.shape)}, "
                         f"{tuple(pose.shape)}, {tuple(intrinsics.shape)}, {tuple(intrinsics_inv.shape)}")
    cam_coords = pixel2cam(depth, intrinsics_inv)
    proj = intrinsics.bmm(pose.to(intrinsics.device))
    grid = cam2pixel(cam_coords, proj[:, :, :3], proj[:, :, -1:], padding_mode)
    return F.grid_sample(feat, grid, padding_mode=padding_mode, align_corners=True)


# ----------------------------------------------------------------------------------------------------------------------
# building blocks (names and nesting are the state-dict keys)
# ----------------------------------------------------------------------------------------------------------------------
def convbn(in_planes, out_planes, kernel_size, stride, pad, dilation):
    return nn.Sequential(nn.Conv2d(in_planes, out_planes, kernel_size=kernel_size, stride=stride, padding=dilation if dilation > 1 else pad,
                                   dilation=dilation, bias=False),
                         nn.BatchNorm2d(out_planes))


def convbn_3d(in_planes, out_planes, kernel_size, stride, pad):
    return nn.Sequential(nn.Conv3d(in_planes, out_planes, kernel_size=kernel_size, padding=pad, stride=stride, bias=False),
                         nn.BatchNorm3d(out_planes))


def convtext(in_planes, out_planes, kernel_size=3, stride=1, dilation=1):
    return nn.Sequential(nn.Conv2d(in_planes, out_planes, kernel_size=kernel_size, stride=stride, dilation=dilation,
                                   padding=((kernel_size - 1) * dilation) // 2, bias=False),
                         nn.LeakyReLU(0.1, inplace=True))


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride, downsample, pad, dilation):
        super().__init__()
        self.conv1 = nn.Sequential(convbn(inplanes, planes, 3, stride, pad, dilation), nn.ReLU(inplace=True))
        self.conv2 = convbn(planes, planes, 3, 1, pad, dilation)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        out = self.conv2(self.conv1(x))
        if self.downsample is not None:
            x = self.downsample(x)
        out += x
        return out


class disparityregression(nn.Module):
    """sum_i x[:, i] * i over the plane axis of [B,maxdisp,H,W] probabilities."""

    def __init__(self, maxdisp):
        super().__init__()
        self.maxdisp = maxdisp

    def forward(self, x):
        disp = torch.arange(self.maxdisp, device=x.device).to(x.dtype).view(1, self.maxdisp, 1, 1)
        return torch.sum(x * disp, 1)


class feature_extraction(nn.Module):
    """The quarter-resolution 32-channel feature extractor with its four pooling branches."""

    def __init__(self):
        super().__init__()
        self.inplanes = 32
        self.firstconv = nn.Sequential(convbn(3, 32, 3, 2, 1, 1), nn.ReLU(inplace=True),
                                       convbn(32, 32, 3, 1, 1, 1), nn.ReLU(inplace=True),
                                       convbn(32, 32, 3, 1, 1, 1), nn.ReLU(inplace=True))
        self.layer1 = self._make_layer(BasicBlock, 32, 3, 1, 1, 1)
        self.layer2 = self._make_layer(BasicBlock, 64, 16, 2, 1, 1)
        self.layer3 = self._make_layer(BasicBlock, 128, 3, 1, 1, 1)
        self.layer4 = self._make_layer(BasicBlock, 128, 3, 1, 1, 2)
        for name, size in (("branch1", 32), ("branch2", 16), ("branch3", 8), ("branch4", 4)):
            setattr(self, name, nn.Sequential(nn.AvgPool2d((size, size), stride=(size, size)), convbn(128, 32, 1, 1, 0, 1), nn.ReLU(inplace=True)))
        self.lastconv = nn.Sequential(convbn(320, 128, 3, 1, 1, 1), nn.ReLU(inplace=True),
                                      nn.Conv2d(128, 32, kernel_size=1, padding=0, stride=1, bias=False))

    def _make_layer(self, block, planes, blocks, stride, pad, dilation):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * block.expansion, kernel_size=1, stride=stride, bias=False),
                                       nn.BatchNorm2d(planes * block.expansion))
        layers = [block(self.inplanes, planes, stride, downsample, pad, dilation)]
        self.inplanes = planes * block.expansion
        layers += [block(self.inplanes, planes, 1, None, pad, dilation) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    def forward(self, x):
        raw = self.layer2(self.layer1(self.firstconv(x)))
        skip = self.layer4(self.layer3(raw))
        size = (skip.shape[2], skip.shape[3])
        b1, b2, b3, b4 = (F.interpolate(branch(skip), size, mode="bilinear", align_corners=False)
                          for branch in (self.branch1, self.branch2, self.branch3, self.branch4))
        return self.lastconv(torch.cat((raw, skip, b4, b3, b2, b1), 1))


# ----------------------------------------------------------------------------------------------------------------------
# the network
# ----------------------------------------------------------------------------------------------------------------------
class PSNet(nn.Module):
    def __init__(self, nlabel, mindepth):
        super().__init__()
        self.nlabel = nlabel
        self.mindepth = mindepth
        self.route = "auto"      # "auto" | "fused" | "plain": see forward

        self.feature_extraction = feature_extraction()
        self.convs = nn.Sequential(convtext(33, 128, 3, 1, 1), convtext(128, 128, 3, 1, 2), convtext(128, 128, 3, 1, 4),
                                   convtext(128, 96, 3, 1, 8), convtext(96, 64, 3, 1, 16), convtext(64, 32, 3, 1, 1), convtext(32, 1, 3, 1, 1))
        self.dres0 = nn.Sequential(convbn_3d(64, 32, 3, 1, 1), nn.ReLU(inplace=True), convbn_3d(32, 32, 3, 1, 1), nn.ReLU(inplace=True))
        for name in ("dres1", "dres2", "dres3", "dres4"):
            setattr(self, name, nn.Sequential(convbn_3d(32, 32, 3, 1, 1), nn.ReLU(inplace=True), convbn_3d(32, 32, 3, 1, 1)))
        self.classify = nn.Sequential(convbn_3d(32, 32, 3, 1, 1), nn.ReLU(inplace=True),
                                      nn.Conv3d(32, 1, kernel_size=3, padding=1, stride=1, bias=False))

        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Conv3d)):
                n = math.prod(m.kernel_size) * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2.0 / n))
            elif isinstance(m, (nn.BatchNorm2d, nn.BatchNorm3d)):
                m.weight.data.fill_(1)
                m.bias.data.zero_()

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
                nn.init.xavier_uniform_(m.weight.data)
                if m.bias is not None:
                    m.bias.data.zero_()

    def train(self, mode=True):
        """BatchNorm stays frozen (eval mode, no gradients to its affine parameters) whatever ``mode`` is."""
        super().train(mode)
        self.apply(freeze_batchnorm)
        return self

    # ---- pieces shared by the two routes ---------------------------------------------------------------------------------------
    @staticmethod
    def quarter_intrinsics(intrinsics, intrinsics_inv):
        K4, Kinv4 = intrinsics.clone(), intrinsics_inv.clone()
        K4[:, :2, :] = K4[:, :2, :] / 4
        Kinv4[:, :2, :2] = Kinv4[:, :2, :2] * 4
        return K4, Kinv4

    def plane_volume(self, ref_fea, target_fea, pose, K4, Kinv4):
        """[B,2C,nlabel,h,w] with torch operations, plane by plane (the plain route; dvmvs::dps_volume is the fused one)."""
        b, c, h, w = ref_fea.shape
        disp2depth = torch.ones((b, h, w), dtype=ref_fea.dtype, device=ref_fea.device) * self.mindepth * self.nlabel
        cost = torch.zeros((b, 2 * c, self.nlabel, h, w), dtype=ref_fea.dtype, device=ref_fea.device)
        for i in range(self.nlabel):
            depth = torch.div(disp2depth, i + 1e-16)
            cost[:, :c, i] = ref_fea
            cost[:, c:, i] = inverse_warp(target_fea, depth, pose, K4, Kinv4)
        return cost

    def regularise(self, cost):
        """The 3-D convolutions: [B,2C,nlabel,h,w] -> plane costs [B,1,nlabel,h,w]."""
        cost0 = self.dres0(cost)
        cost0 = self.dres1(cost0) + cost0
        cost0 = self.dres2(cost0) + cost0
        cost0 = self.dres3(cost0) + cost0
        cost0 = self.dres4(cost0) + cost0
        return self.classify(cost0)

    def context_per_plane(self, ref_fea, costs):
        """The context network plane by plane, as the reference runs it (nlabel batch-B calls)."""
        costss = torch.zeros_like(costs)
        for i in range(self.nlabel):
            costt = costs[:, :, i]
            costss[:, :, i] = self.convs(torch.cat([ref_fea, costt], 1)) + costt
        return costss

    def context_batched(self, ref_fea, costs):
        """The same network once on all planes as a batch of B * nlabel: the planes are independent."""
        b, c, h, w = ref_fea.shape
        planes = costs[:, 0].reshape(b * self.nlabel, 1, h, w)
        fea = ref_fea.unsqueeze(1).expand(b, self.nlabel, c, h, w).reshape(b * self.nlabel, c, h, w)
        return (self.convs(torch.cat([fea, planes], 1)) + planes).view(b, 1, self.nlabel, h, w)

    def regress(self, costs, height, width):
        """(depth [B,1,H,W], pred [B,H,W]) with torch operations: up-sample the costs, softmax over the planes, expectation."""
        up = F.interpolate(costs, [self.nlabel, height, width], mode="trilinear", align_corners=False)
        pred = disparityregression(self.nlabel)(F.softmax(torch.squeeze(up, 1), dim=1))
        return self.mindepth * self.nlabel / (pred.unsqueeze(1) + 1e-16), pred

    # ---- forward ------------------------------------------------------------------------------------------------------------------
    def _use_fused(self, tensors):
        if self.route != "auto":
            return self.route == "fused"
        on_gpu = all(t.is_cuda for t in tensors)
        needs_grad = torch.is_grad_enabled() and (any(t.requires_grad for t in tensors) or any(p.requires_grad for p in self.parameters()))
        return on_gpu and not needs_grad

    def forward(self, ref, targets, pose, intrinsics, intrinsics_inv, outputs=None):
        """(depth0, depth), each [B,1,H,W].  ``targets`` and ``pose`` are lists over the measurement frames (pose[j] [B,3,4] maps the
        reference camera to measurement camera j).  ``outputs`` (a dict) receives the quarter-resolution reference features, ``costs``,
        ``costss``, ``pred0`` and ``pred``."""
        fused = self._use_fused([ref, intrinsics, intrinsics_inv, *targets, *pose])
        if fused:
            from dvmvs.hip import ops           # raises if the HIP library is missing: no fallback
        K4, Kinv4 = self.quarter_intrinsics(intrinsics, intrinsics_inv)
        ref_fea = self.feature_extraction(ref)
        costs = None
        for j, target in enumerate(targets):
            target_fea = self.feature_extraction(target)
            if fused:
                cost = ops.dps_volume(ref_fea, target_fea, pose[j], K4, Kinv4, self.nlabel, self.mindepth)
            else:
                cost = self.plane_volume(ref_fea, target_fea, pose[j], K4, Kinv4)
            cost0 = self.regularise(cost)
            costs = cost0 if j == 0 else costs + cost0
        costs = costs / len(targets)
        height, width = ref.shape[2], ref.shape[3]
        if fused:
            costss = self.context_batched(ref_fea, costs)
            depth0, pred0 = ops.dps_regress(costs, height, width, self.mindepth, outputs is not None)
            depth, pred = ops.dps_regress(costss, height, width, self.mindepth, outputs is not None)
        else:
            costss = self.context_per_plane(ref_fea, costs)
            depth0, pred0 = self.regress(costs, height, width)
            depth, pred = self.regress(costss, height, width)
        if outputs is not None:
            outputs.update(features=ref_fea, costs=costs, costss=costss, pred0=pred0, pred=pred)
        return depth0, depth

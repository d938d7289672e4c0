"""Encoder and decoder shared by the MVDepthNet and GP-MVS baselines (the two reference packages define the same modules).

Module and parameter names are those of the reference's dvmvs/baselines/{mvdepthnet,gpmvs}/{encoder,decoder}.py, so the
published checkpoints load unchanged.  The convolutions run on MIOpen through torch: their 7x7 and 5x5 layers at 256x320 fit
neither of this project's convolution kernels.
"""
import torch
from torch import nn

from dvmvs.utils import freeze_batchnorm


def _conv_bn_relu(cin, cout, k, stride=1):
    return [nn.Conv2d(cin, cout, k, padding=(k - 1) // 2, stride=stride, bias=False), nn.BatchNorm2d(cout), nn.ReLU()]


def down_conv_layer(cin, cout, k):
    """conv (stride 1) + BN + ReLU, conv (stride 2) + BN + ReLU: indices 0..5."""
    return nn.Sequential(*_conv_bn_relu(cin, cout, k), *_conv_bn_relu(cout, cout, k, stride=2))


def conv_layer(cin, cout, k):
    return nn.Sequential(*_conv_bn_relu(cin, cout, k))


def up_conv_layer(cin, cout, k):
    """2x bilinear up-sampling (align_corners=True), then conv + BN + ReLU: the convolution is index 1."""
    return nn.Sequential(nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True), *_conv_bn_relu(cin, cout, k))


def depth_layer(cin):
    return nn.Sequential(nn.Conv2d(cin, 1, 3, padding=1), nn.Sigmoid())


class _FrozenBN(nn.Module):
    def train(self, mode=True):
        """train() keeps every BatchNorm in eval mode with frozen affine parameters, as the reference does."""
        super().train(mode)
        self.apply(freeze_batchnorm)
        return self


class Encoder(_FrozenBN):
    """Input: the reference image (3 channels) and the 64-plane SAD cost volume, 67 channels in all, at 256x320."""

    def __init__(self):
        super().__init__()
        self.conv1 = down_conv_layer(67, 128, 7)
        self.conv2 = down_conv_layer(128, 256, 5)
        self.conv3 = down_conv_layer(256, 512, 3)
        self.conv4 = down_conv_layer(512, 512, 3)
        self.conv5 = down_conv_layer(512, 512, 3)

    def forward(self, image, plane_sweep_volume):
        return self.forward_fused(torch.cat((image, plane_sweep_volume), 1))

    def forward_fused(self, x):
        """``x`` = cat(image, cost volume) as one tensor: what dvmvs::rgb_sweep writes with copy_image.  Returns
        [conv5, conv4, conv3, conv2, conv1]."""
        conv1 = self.conv1(x)
        conv2 = self.conv2(conv1)
        conv3 = self.conv3(conv2)
        conv4 = self.conv4(conv3)
        conv5 = self.conv5(conv4)
        return [conv5, conv4, conv3, conv2, conv1]


class Decoder(_FrozenBN):
    """Returns [disp1, disp2, disp3, disp4]: inverse depth in (0, 2) at full, 1/2, 1/4 and 1/8 resolution."""

    def __init__(self):
        super().__init__()
        self.upconv5 = up_conv_layer(512, 512, 3)
        self.iconv5 = conv_layer(1024, 512, 3)
        self.upconv4 = up_conv_layer(512, 512, 3)
        self.iconv4 = conv_layer(1024, 512, 3)
        self.disp4 = depth_layer(512)
        self.upconv3 = up_conv_layer(512, 256, 3)
        self.iconv3 = conv_layer(513, 256, 3)
        self.disp3 = depth_layer(256)
        self.upconv2 = up_conv_layer(256, 128, 3)
        self.iconv2 = conv_layer(257, 128, 3)
        self.disp2 = depth_layer(128)
        self.upconv1 = up_conv_layer(128, 64, 3)
        self.iconv1 = conv_layer(65, 64, 3)
        self.disp1 = depth_layer(64)

    def forward(self, conv5, conv4, conv3, conv2, conv1):
        up = nn.functional.interpolate       # nearest, as the reference's F.interpolate(disp, scale_factor=2)
        iconv5 = self.iconv5(torch.cat((self.upconv5(conv5), conv4), 1))
        iconv4 = self.iconv4(torch.cat((self.upconv4(iconv5), conv3), 1))
        disp4 = 2.0 * self.disp4(iconv4)
        iconv3 = self.iconv3(torch.cat((self.upconv3(iconv4), conv2, up(disp4, scale_factor=2)), 1))
        disp3 = 2.0 * self.disp3(iconv3)
        iconv2 = self.iconv2(torch.cat((self.upconv2(iconv3), conv1, up(disp3, scale_factor=2)), 1))
        disp2 = 2.0 * self.disp2(iconv2)
        iconv1 = self.iconv1(torch.cat((self.upconv1(iconv2), up(disp2, scale_factor=2)), 1))
        disp1 = 2.0 * self.disp1(iconv1)
        return [disp1, disp2, disp3, disp4]

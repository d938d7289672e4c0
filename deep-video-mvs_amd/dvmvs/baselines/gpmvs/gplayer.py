"""GP-MVS's Gaussian-process layer (the reference's dvmvs/baselines/gpmvs/gplayer.py): three log-hyper-parameters of a Matern 3/2
kernel over pose distances.  ``forward`` is the batched form used in training (plain torch); inference runs the same prior as
a Kalman filter over frames (dvmvs.baselines.runner.GPFilter, dvmvs::gp_filter_step)."""
import math

import torch

from dvmvs.utils import freeze_batchnorm


class GPlayer(torch.nn.Module):
    def __init__(self, device):
        super().__init__()
        self.gamma2 = torch.nn.Parameter(torch.randn(1).to(device).float(), requires_grad=True)
        self.ell = torch.nn.Parameter(torch.randn(1).to(device).float(), requires_grad=True)
        self.sigma2 = torch.nn.Parameter(torch.randn(1).to(device).float(), requires_grad=True)
        self.device = device

    def forward(self, D, Y):
        """D: [batch, latents, latents] pose distances; Y: [batch, latents, C, H, W] encoder outputs.  Returns relu(K (K + s I)^-1 Y)
        as [batch, latents, C*H*W]."""
        batch, latents = Y.shape[:2]
        Y = Y.view(batch, latents, -1).float()
        D = D.to(self.device).float()
        scaled = math.sqrt(3) * D / torch.exp(self.ell)
        K = torch.exp(self.gamma2) * (1 + scaled) * torch.exp(-scaled)
        eye = torch.eye(latents, device=self.device, dtype=torch.float32).expand(batch, latents, latents)
        C = K + torch.exp(self.sigma2) * eye
        return torch.relu(K.bmm(C.inverse()).bmm(Y))

    def train(self, mode=True):
        super().train(mode)
        self.apply(freeze_batchnorm)
        return self

"""RunningMoments: a read-only view of a (count, mean[D], M2[D]) float64 block that pf_traj_stats keeps up to date on the device
(BatchEngine.obs_moments, BatchEngine.ret_moments). Nothing here synchronises: every property is a small float32 device tensor
computed from the block when it is read."""
from __future__ import annotations

import torch


class RunningMoments:
    def __init__(self, block):
        if not torch.is_tensor(block) or block.dtype != torch.float64 or block.dim() != 1 or block.numel() < 3 or block.numel() % 2 != 1:
            raise ValueError("block must be a float64 tensor of shape (1 + 2 D,): count, mean[D], M2[D]; got "
                             f"{(block.dtype, tuple(block.shape)) if torch.is_tensor(block) else type(block).__name__}")
        self.block = block
        self.dim = (block.numel() - 1) // 2

    @property
    def count(self):
        """[] float32: how many samples the block holds."""
        return self.block[0].float()

    @property
    def mean(self):
        """[D] float32."""
        return self.block[1:1 + self.dim].float()

    @property
    def var(self):
        """[D] float32: M2 / count, the population variance as gymnasium's normalisers keep it; 1 while count < 2."""
        n = self.block[0]
        return torch.where(n < 2.0, torch.ones_like(self.block[1 + self.dim:]), self.block[1 + self.dim:] / n.clamp_min(1.0)).float()

    def std(self, eps: float = 1e-8):
        """[D] float32: sqrt(var + eps)."""
        return (self.var + eps).sqrt()

    def __repr__(self):
        return f"RunningMoments(dim={self.dim})"

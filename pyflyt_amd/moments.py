"""RunningMoments: a read-only view of a (count, mean[D], M2[D]) float64 block that pf_traj_stats keeps up to date on the device
(BatchEngine.obs_moments, BatchEngine.ret_moments). Nothing here synchronises: every property is a small float32 device tensor
computed from the block when it is read.

EpisodeStats: what an env façade with collect(stats=True) shows of its engine's accounting -- obs_rms, ret_rms and
episode_summary_dict() --, one copy for the vector envs and the multi-agent envs."""
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


class EpisodeStats:
    """Mixin of the env façades whose collect() takes stats= / normalize_reward=: needs `engine` (a BatchEngine)."""

    @property
    def obs_rms(self):
        """RunningMoments of the observation columns the policy saw on valid steps, updated by collect(stats=True)."""
        return RunningMoments(self.engine.obs_moments)

    @property
    def ret_rms(self):
        """RunningMoments (dim 1) of the discounted return over the valid steps, updated by collect(stats=True)."""
        return RunningMoments(self.engine.ret_moments)

    def episode_summary_dict(self):
        """The last collect(stats=True)'s episode_summary as Python numbers (THE place that synchronises with the device): episodes,
        return_mean / return_std / return_min / return_max, length_mean, terminated, truncated; the means are nan when no episode
        finished in that call."""
        c, s1, s2, lo, hi, ln, te, tr = self.engine._traj_state()["summary"].tolist()
        mean = s1 / c if c else float("nan")
        return dict(episodes=int(c), return_mean=mean, return_std=max(s2 / c - mean * mean, 0.0) ** 0.5 if c else float("nan"), return_min=lo,
                    return_max=hi, length_mean=ln / c if c else float("nan"), terminated=int(te), truncated=int(tr))

    def _adopt_moments(self, moments):
        """After reset(seed=other) built a new engine: `moments` = the old engine's made_moments(), taken before it was closed.
        traj_stats' running moments outlive the engine; its carries do not."""
        if moments is not None:
            self.engine.obs_moments.copy_(moments[0])
            self.engine.ret_moments.copy_(moments[1])

"""ShardedVecEnv: make_vec(id, num_envs, devices=[...]) -- the lanes of ONE vector env cut into contiguous slices, one ordinary
vector env per device (dist.strong_shard's slices, the same seed, lane_offset = the slice's first lane: the counter-based draws are
keyed by the global lane, so the shards together reproduce the whole env bit for bit). One process, one engine and one stream per
device, no collective, no gather: every call issues all shards' work before it touches a result and returns per-shard lists.
What joins the shards is small and explicit: the running normalisers of collect(stats=True) (pf_moments_merge on devices[0]) and
the gradient (pyflyt_amd.ppo_grad_sharded). DESIGN.md section 32."""
from __future__ import annotations

import torch

from .. import _lib as L
from ..dist import strong_shard
from ..moments import RunningMoments


class ShardedVecEnv:
    def __init__(self, env_class, num_envs: int, devices, *, lane_offset: int = 0, **kwargs):
        try:
            self.devices = [torch.device(d) for d in devices]
        except TypeError:
            raise ValueError(f"devices must be a list of devices, got {type(devices).__name__}") from None
        G = len(self.devices)
        if G < 1:
            raise ValueError("devices must name at least one device (one shard per entry; a device may be named more than once)")
        if isinstance(num_envs, bool) or not isinstance(num_envs, int) or num_envs < G:
            raise ValueError(f"num_envs must be an int of at least one env per device ({G}), got {num_envs!r}")
        if "device" in kwargs:
            raise ValueError("device comes with a plain make_vec; with devices= every shard lives on its entry of the list")
        self.num_envs = num_envs
        self.slices = [strong_shard(num_envs, g, G) for g in range(G)]
        self.shards = [env_class(s.lanes, device=d, lane_offset=int(lane_offset) + s.lane_offset, **kwargs) for s, d in zip(self.slices, self.devices)]
        first = self.shards[0]
        self.single_action_space, self.single_observation_space = first.single_action_space, first.single_observation_space
        self.metadata = dict(first.metadata)
        self._moments = None  # (obs [1 + 2 D], ret [3]) float64 on devices[0]: the running normalisers of ALL shards, made at first use

    # ------------------------------------------------------------------ gymnasium.vector's calls, per shard
    def reset(self, *, seed: int | None = None, options: dict | None = None):
        """Every shard's reset(seed=, options=); returns ([obs per shard], [infos per shard]). options['reset_mask'] is not split
        over the shards: reset a shard's lanes through self.shards[g]."""
        if options and options.get("reset_mask") is not None:
            raise ValueError("a reset_mask is a shard's own: call shards[g].reset(options=...) with that shard's lanes")
        out = [s.reset(seed=seed, options=options) for s in self.shards]
        return [o for o, _ in out], [i for _, i in out]

    def _per_shard(self, name, xs):
        if not isinstance(xs, (list, tuple)) or len(xs) != len(self.shards):
            raise ValueError(f"{name} must be a list with one entry per shard ({len(self.shards)}), got {len(xs) if isinstance(xs, (list, tuple)) else type(xs).__name__}")
        return list(xs)

    def step(self, actions):
        """actions: a list, one [lanes_g, action width] tensor per shard. Returns the shards' 5-tuples as five lists."""
        out = [s.step(a) for s, a in zip(self.shards, self._per_shard("actions", actions))]
        return tuple([o[i] for o in out] for i in range(5))

    def sample_actions(self, step_index: int = 0):
        return [s.sample_actions(step_index) for s in self.shards]

    def rollout(self, policies, k_steps: int, **kw):
        """Every shard's rollout(policies[g], k_steps, ...) with its own policy (on its device); a list of the shards' results."""
        return [s.rollout(p, k_steps, **kw) for s, p in zip(self.shards, self._per_shard("policies", policies))]

    def collect(self, policies, value_fns, k_steps: int, gamma: float = 0.99, lam: float = 0.95, stats: bool = False, normalize_reward: bool = False,
                fused=None, outcomes: bool = False):
        """Every shard's collect() -- policies and value_fns are lists, one entry per shard, on the shard's device -- as a list of
        batch dicts. With stats the running normalisers are those of ALL shards: each shard's pf_traj_stats runs on emptied blocks
        (so they hold this batch only, about the shift 0), the previous global blocks and the G batch blocks are merged on
        devices[0] (pf_moments_merge, in shard order), and the merged blocks are written back into every shard's engine before the
        second half of its collect -- so normalize_reward scales every shard's reward by the same number, and shards[g].obs_rms /
        .ret_rms read the global moments too."""
        policies, value_fns = self._per_shard("policies", policies), self._per_shard("value_fns", value_fns)
        want = [s._collect_args(p, v, gamma, lam, stats, normalize_reward, outcomes) for s, p, v in zip(self.shards, policies, value_fns)][0]
        k, trajs = int(k_steps), []
        for s in self.shards:
            if not s.engine._fused_policy(fused, outcomes):
                s.engine._check_stepwise()
        for s, p in zip(self.shards, policies):  # the closed loops of all shards first
            eng, episode_start = s.engine, None
            if eng.params.autoreset == L.AUTORESET_NEXT_STEP:
                episode_start = (eng.flags() & (L.F_TERMINATED | L.F_TRUNCATED)) != 0
            t = eng.collect_rollout(p, k, step_index0=s._policy_step, fused=fused, outcomes=outcomes)
            s._after_policy_steps(k)
            trajs.append((t, episode_start))
        heads = []
        for s, v, (t, episode_start) in zip(self.shards, value_fns, trajs):
            if want:
                s.engine.reset_moments()
            heads.append(s._collect_head(t, v, gamma, want, episode_start, None, outcomes))
        if want:
            self._merge_moments()
        return [s._collect_tail(t, h, p, gamma, lam, want and normalize_reward, s._infos_obj, episode_start, None)
                for s, p, h, (t, episode_start) in zip(self.shards, policies, heads, trajs)]

    # ------------------------------------------------------------------ the normalisers of all shards
    def _global_moments(self):
        if self._moments is None:
            D, dev = self.shards[0].engine.obs_dim, self.devices[0]
            self._moments = (torch.zeros(1 + 2 * D, dtype=torch.float64, device=dev), torch.zeros(3, dtype=torch.float64, device=dev))
        return self._moments

    def _merge_moments(self):
        dev0, eng0 = self.devices[0], self.shards[0].engine
        glob = self._global_moments()
        for which, dst in enumerate(glob):  # (copy=True: a block on devices[0] is an engine's own, rewritten below)
            eng0.moments_merge(dst, [s.engine.made_moments()[which].to(dev0, non_blocking=True, copy=True) for s in self.shards])
        for s in self.shards:
            for which, dst in enumerate(s.engine.made_moments()):
                dst.copy_(glob[which], non_blocking=True)

    @property
    def obs_rms(self):
        """RunningMoments of the observation columns over the valid steps of ALL shards (on devices[0])."""
        return RunningMoments(self._global_moments()[0])

    @property
    def ret_rms(self):
        return RunningMoments(self._global_moments()[1])

    def episode_summary_dict(self):
        """EpisodeStats.episode_summary_dict over all shards' last collect(stats=True): counts and sums added in shard order, the
        minimum and maximum taken. Synchronises with every device."""
        rows = [s.engine._traj_state()["summary"].tolist() for s in self.shards]
        c, s1, s2, ln, te, tr = (sum(r[i] for r in rows) for i in (0, 1, 2, 5, 6, 7))
        lo, hi = min(r[3] for r in rows), max(r[4] for r in rows)
        mean = s1 / c if c else float("nan")
        return dict(episodes=int(c), return_mean=mean, return_std=max(s2 / c - mean * mean, 0.0) ** 0.5 if c else float("nan"), return_min=lo,
                    return_max=hi, length_mean=ln / c if c else float("nan"), terminated=int(te), truncated=int(tr))

    def close(self):
        for s in self.shards:
            s.close()

"""rollout() and collect() of the multi-agent façades: the closed loop of BatchEngine.rollout_policy_worlds / collect_rollout_worlds
(pf_policy_act, pf_env_step, pf_world_sync, pf_env_reset per step: a copy of the env whose agents have all finished is reset on the
device) and the PPO batch pf_gae makes of it. One copy of the code for both envs; each env's rollout() / collect() says what is its own.

The batch is flat: a tensor is [k, n, ...] with n = num_envs * agents and lane = copy * agents + agent, so t.view(k, num_envs, agents,
...) reads it per copy and agent. `valid` is pf_world_sync's: False on the steps an agent sat out after its episode had ended, on
the step that reset its copy, and on an opponent's lanes. pf_gae's own `valid` is all ones under auto-reset OFF and is not returned.

collect(stats=True) hands that `valid` to pf_traj_stats_masked (BatchEngine.traj_stats(valid=...)): the episode accounting and the running
moments behind obs_rms / ret_rms (moments.EpisodeStats, the vector envs' copy) see the valid steps and nothing else.
"""
from __future__ import annotations

import torch

from .. import _checks as K
from ..engine import BatchEngine
from ..gym_envs.vector_envs import LazyInfos
from ..moments import EpisodeStats


class WorldRollout(EpisodeStats):
    """Mixin of MAFixedwingDogfightEnv and MAQuadXHoverEnv: needs engine, num_possible_agents, possible_agents, agents, and
    _flat_infos() (the infos of the last step over the flat lanes)."""

    _needs_reset = True  # until the first reset()
    _policy_step = 0  # the step index that keys the policies' exploration noise: advances by k per call, restarts with reset(seed=...)

    def _world_args(self, opponent):
        """(opponent, opponent_lanes) for the engine: none here; the dogfight has team 1."""
        if opponent is not None:
            raise ValueError("this env has no opponent (one team)")
        return None, None

    def _after_worlds(self, k):
        self._policy_step = (self._policy_step + k) & 0xFFFFFFFF
        self.step_count += k
        self.agents = self.possible_agents[:]  # (as after reset_envs: finished copies restart on the device, no agent is culled for good)

    def _world_rollout(self, policy, k_steps, opponent, store_mean):
        if self._needs_reset:
            raise RuntimeError("call reset() before rollout()")
        k = int(k_steps)
        opponent, lanes = self._world_args(opponent)
        out = self.engine.rollout_policy_worlds(policy, k, self.num_possible_agents, step_index0=self._policy_step, opponent=opponent,
                                                opponent_lanes=lanes, store_mean=bool(store_mean))
        self._after_worlds(k)
        return out

    def _world_collect(self, policy, value_fn, k_steps, gamma, lam, opponent, stats=False, normalize_reward=False):
        if self._needs_reset:
            raise RuntimeError("call reset() before collect()")
        K.boolean(stats, "stats")
        K.boolean(normalize_reward, "normalize_reward")
        stats = stats or normalize_reward
        BatchEngine._check_policy(policy)
        if not callable(value_fn):
            raise ValueError(f"value_fn must be callable (a float32 [M, D] tensor -> [M] or [M, 1]), got {type(value_fn).__name__}")
        K.unit_interval(gamma, "gamma")
        K.unit_interval(lam, "lam")
        eng, k = self.engine, int(k_steps)
        opponent, lanes = self._world_args(opponent)
        t = eng.collect_rollout_worlds(policy, k, self.num_possible_agents, step_index0=self._policy_step, opponent=opponent, opponent_lanes=lanes)
        self._after_worlds(k)
        rows = t["obs_all"]
        m = rows.shape[0] * rows.shape[1]
        with torch.no_grad():
            v = value_fn(rows.view(m, eng.obs_dim))
        if not torch.is_tensor(v) or v.dtype != torch.float32 or tuple(v.shape) not in ((m,), (m, 1)):
            raise ValueError(f"value_fn must map the float32 {(m, eng.obs_dim)} observations to a float32 tensor of shape {(m,)} or {(m, 1)}, "
                             f"got {(v.dtype, tuple(v.shape)) if torch.is_tensor(v) else type(v).__name__}")
        values = v.reshape(rows.shape[0], rows.shape[1]).contiguous()
        has_std = policy.log_std is not None
        extra, reward = {}, t["reward"]
        if stats:
            ep_ret, ep_len, summary = eng.traj_stats(t["reward"], t["terminated"], t["truncated"], gamma=gamma, obs=t["obs_all"][:-1], valid=t["valid"])
            extra = dict(episode_return=ep_ret, episode_length=ep_len, episode_summary=summary)
            if normalize_reward:
                reward = extra["reward_scaled"] = t["reward"] / (self.ret_rms.var + 1e-8).sqrt()
        adv, ret, logp, _ = eng.gae(reward, t["terminated"], t["truncated"], values, gamma=gamma, lam=lam,
                                    actions=t["actions"] if has_std else None, mean=t["mean"] if has_std else None,
                                    log_std=policy.log_std if has_std else None)
        return dict(obs=t["obs_all"][:-1], actions=t["actions"], mean=t["mean"], logp=logp, values=values[:-1], advantages=adv, returns=ret,
                    valid=t["valid"], reward=t["reward"], terminated=t["terminated"], truncated=t["truncated"], last_value=values[-1],
                    infos=LazyInfos(self._flat_infos()), **extra)

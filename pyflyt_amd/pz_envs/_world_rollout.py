"""What the multi-agent façades share. Their PettingZoo boilerplate: the agent names, the spaces, the per-agent views of a flat tensor.
And their rollout() and collect(): the closed loop of BatchEngine.rollout_policy_worlds / collect_rollout_worlds (pf_policy_act,
pf_env_step, pf_world_sync, pf_env_reset per step: a copy of the env whose agents have all finished is reset on the device) and the PPO
batch pf_gae makes of it, assembled by the vector envs' code (_collect.ClosedLoopEnv). One copy for both envs; each env's rollout() /
collect() says what is its own.

The batch is flat: a tensor is [k, n, ...] with n = num_envs * agents and lane = copy * agents + agent, so t.view(k, num_envs, agents,
...) reads it per copy and agent. `valid` is pf_world_sync's: False on the steps an agent sat out after its episode had ended, on
the step that reset its copy, and on an opponent's lanes. pf_gae's own `valid` is all ones under auto-reset OFF and is not returned.

rollout(outcomes=True) / collect(outcomes=True) add pf_episode_outcomes to every step, between pf_world_sync and the reset: outcome
[k, n] uint8 says why each episode ended, outcome_counts [G, 16] int64 counts this call's episodes and finished copies per group
(episode_outcomes_dict() reads a block back by name; _collect.ClosedLoopEnv).

collect(stats=True) hands that `valid` to pf_traj_stats_masked (BatchEngine.traj_stats(valid=...)): the episode accounting and the running
moments behind obs_rms / ret_rms (moments.EpisodeStats, the vector envs' copy) see the valid steps and nothing else.
"""
from __future__ import annotations

from typing import Any

import torch

from .._collect import ClosedLoopEnv
from ..gym_envs.vector_envs import LazyInfos


class WorldRollout(ClosedLoopEnv):
    """Base of MAFixedwingDogfightEnv and MAQuadXHoverEnv: needs engine, _action_space, _observation_space, step_count and
    _flat_infos() (the infos of the last step over the flat lanes)."""

    @staticmethod
    def _no_render(render_mode):
        if render_mode is not None:
            raise ValueError("rendering is out of scope for the batched GPU path")

    @staticmethod
    def _check_agent_hz(agent_hz):
        if 120 % agent_hz != 0:  # ma_quadx_base_env.py:60-65, ma_fixedwing_base_env.py:52-57
            lowest, highest = int(120 / (int(120 / agent_hz) + 1)), int(120 / int(120 / agent_hz))
            raise AssertionError(f"`agent_hz` must be round denominator of 120, try {lowest} or {highest}.")

    def _init_agents(self, count, num_envs, device):
        """`count` agents "uav_i" in each of `num_envs` copies."""
        self.num_possible_agents = count
        self.possible_agents = ["uav_" + str(r) for r in range(count)]
        self.agent_name_mapping = dict(zip(self.possible_agents, range(count)))
        self.agents: list[str] = []
        self.num_envs = int(num_envs)
        self.device = torch.device(device)

    def observation_space(self, agent: Any = None):
        return self._observation_space

    def action_space(self, agent: Any = None):
        return self._action_space

    def _split(self, t):
        """[E*A, ...] -> per-agent views [E, ...] (squeezed when E == 1)."""
        A, E = self.num_possible_agents, self.num_envs
        t = t.view(E, A, *t.shape[1:])
        return [t[:, i].squeeze(0) if E == 1 else t[:, i] for i in range(A)]

    # ------------------------------------------------------------------ closed-loop rollouts
    def _world_args(self, opponent):
        """(opponent, opponent_lanes, group, n_groups) for the engine: no opponent and one group here; the dogfight has team 1, and
        a pool of opponents cuts its copies into one group each."""
        if opponent is not None:
            raise ValueError("this env has no opponent (one team)")
        return None, None, None, 1

    def _after_worlds(self, k):
        self._policy_step = (self._policy_step + k) & 0xFFFFFFFF
        self.step_count += k
        self.agents = self.possible_agents[:]  # (as after reset_envs: finished copies restart on the device, no agent is culled for good)

    def _world_rollout(self, policy, k_steps, opponent, store_mean, outcomes=False, pooled=False):
        if self._needs_reset:
            raise RuntimeError("call reset() before rollout()")
        k = int(k_steps)
        opponent, lanes, group, n_groups = self._world_args(opponent)
        out = self.engine.rollout_policy_worlds(policy, k, self.num_possible_agents, step_index0=self._policy_step, opponent=opponent,
                                                opponent_lanes=lanes, store_mean=bool(store_mean), outcomes=outcomes, group=group, n_groups=n_groups,
                                                pooled=pooled)
        self._after_worlds(k)
        return out

    def _world_collect(self, policy, value_fn, k_steps, gamma, lam, opponent, stats=False, normalize_reward=False, outcomes=False, pooled=False):
        stats = self._collect_args(policy, value_fn, gamma, lam, stats, normalize_reward, outcomes)
        k = int(k_steps)
        opponent, lanes, group, n_groups = self._world_args(opponent)
        t = self.engine.collect_rollout_worlds(policy, k, self.num_possible_agents, step_index0=self._policy_step, opponent=opponent,
                                               opponent_lanes=lanes, outcomes=outcomes, group=group, n_groups=n_groups, pooled=pooled)
        self._after_worlds(k)
        return self._collect_batch(t, policy, value_fn, gamma, lam, stats, normalize_reward, LazyInfos(self._flat_infos()), valid=t["valid"],
                                   outcomes=outcomes)

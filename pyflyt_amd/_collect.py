"""ClosedLoopEnv: what the env façades with rollout() and collect() share -- the vector envs (gym_envs/vector_envs.py) and the
multi-agent envs (pz_envs/_world_rollout.py). One copy of collect()'s argument checks, of the batch it assembles from a trajectory
(value_fn, pf_traj_stats, pf_gae, the result dict) and of the rebuild behind reset(seed=other). Each collect() says what is its own:
how the trajectory is produced, episode_start, which `valid` counts, the infos."""
from __future__ import annotations

import torch

from . import _checks as K
from . import _lib as L
from .engine import BatchEngine
from .moments import EpisodeStats


class ClosedLoopEnv(EpisodeStats):
    """Mixin: needs `engine` (a BatchEngine), `_seed` and `_build(seed)`, which makes a new engine."""

    _needs_reset = True  # until the first reset()
    _policy_step = 0  # the step index that keys the policies' exploration noise: advances by k per call, restarts with reset(seed=...)

    def close(self):
        self.engine.close()

    def _collect_args(self, policy, value_fn, gamma, lam, stats, normalize_reward, outcomes=False):
        """collect()'s refusals, in their order, before anything reads the engine; returns whether pf_traj_stats runs."""
        if self._needs_reset:
            raise RuntimeError("call reset() before collect()")
        K.boolean(stats, "stats")
        K.boolean(normalize_reward, "normalize_reward")
        K.boolean(outcomes, "outcomes")
        BatchEngine._check_policy(policy)
        if not callable(value_fn):
            raise ValueError(f"value_fn must be callable (a float32 [M, D] tensor -> [M] or [M, 1]), got {type(value_fn).__name__}")
        K.unit_interval(gamma, "gamma")
        K.unit_interval(lam, "lam")
        return stats or normalize_reward

    def _collect_batch(self, t, policy, value_fn, gamma, lam, stats, normalize_reward, infos, episode_start=None, valid=None, outcomes=False):
        """The PPO batch of the trajectory `t` (BatchEngine.collect_rollout's dict, or collect_rollout_worlds'): the values of all
        k + 1 observation rows and, where `t` has them (SAME_STEP), of the final_obs rows; with `stats` pf_traj_stats before pf_gae.
        `episode_start` [n]: NEXT_STEP only, for both kernels. `valid` [k, n]: the mask of a trajectory that brings its own
        (pf_world_sync's: pf_traj_stats_masked, and what the batch returns); None = pf_gae's. `outcomes`: the closed loop ran with
        them, and the batch gains outcome [k, n] uint8 and outcome_counts [G, 16] int64.
        Two halves, cut behind pf_traj_stats: a sharded env (gym_envs/sharded.py) merges the shards' running moments between them."""
        head = self._collect_head(t, value_fn, gamma, stats, episode_start, valid, outcomes)
        return self._collect_tail(t, head, policy, gamma, lam, stats and normalize_reward, infos, episode_start, valid)

    def _collect_head(self, t, value_fn, gamma, stats, episode_start, valid, outcomes):
        """_collect_batch up to and including pf_traj_stats: (values, final_values, the batch's extra entries so far)."""
        eng = self.engine

        def value(rows, what):
            m = rows.shape[0] * rows.shape[1]
            v = value_fn(rows.view(m, eng.obs_dim))
            if not torch.is_tensor(v) or v.dtype != torch.float32 or tuple(v.shape) not in ((m,), (m, 1)):
                raise ValueError(f"value_fn must map the float32 {(m, eng.obs_dim)} {what} to a float32 tensor of shape {(m,)} or {(m, 1)}, "
                                 f"got {(v.dtype, tuple(v.shape)) if torch.is_tensor(v) else type(v).__name__}")
            return v.reshape(rows.shape[0], rows.shape[1]).contiguous()

        with torch.no_grad():
            values = value(t["obs_all"], "observations")
            final_values = value(t["final_obs"], "final observations") if t["final_obs"] is not None else None
        extra = {}
        if outcomes:
            extra = dict(outcome=t["outcome"], outcome_counts=t["outcome_counts"])
        if stats:
            ep_ret, ep_len, summary = eng.traj_stats(t["reward"], t["terminated"], t["truncated"], gamma=gamma, episode_start=episode_start,
                                                     obs=t["obs_all"][:-1], valid=valid)
            extra.update(episode_return=ep_ret, episode_length=ep_len, episode_summary=summary)
        return values, final_values, extra

    def _collect_tail(self, t, head, policy, gamma, lam, normalize_reward, infos, episode_start, valid):
        """_collect_batch behind pf_traj_stats: the reward scaled by ret_rms as it stands now, pf_gae, the result dict."""
        eng = self.engine
        values, final_values, extra = head
        has_std = policy.log_std is not None
        reward = t["reward"]
        if normalize_reward:
            reward = extra["reward_scaled"] = t["reward"] / (self.ret_rms.var + 1e-8).sqrt()
        adv, ret, logp, gae_valid = eng.gae(reward, t["terminated"], t["truncated"], values, gamma=gamma, lam=lam, final_values=final_values,
                                            episode_start=episode_start, actions=t["actions"] if has_std else None,
                                            mean=t["mean"] if has_std else None, log_std=policy.log_std if has_std else None)
        return dict(obs=t["obs_all"][:-1], actions=t["actions"], mean=t["mean"], logp=logp, values=values[:-1], advantages=adv, returns=ret,
                    valid=gae_valid if valid is None else valid, reward=t["reward"], terminated=t["terminated"], truncated=t["truncated"],
                    last_value=values[-1], infos=infos, **extra)

    def episode_outcomes_dict(self, counts=None):
        """A block of outcome counts ([G, 16] int64: a batch's outcome_counts; default: that of the last rollout() / collect() with
        outcomes=True) as Python numbers by slot name, one dict per group (THE place that synchronises with the device): episodes,
        terminated, truncated, collision, out_of_bounds, complete (env_complete; the dogfight's team_win), dead, nonfinite,
        second_word_sum (targets reached on the waypoint envs, received hits on the dogfight, 0 elsewhere), clean (ran to the limit
        with no cause bit), and per world: worlds, team0_wins, team1_wins, draws."""
        if counts is None:
            counts = self.engine._oc_last
            if counts is None:
                raise RuntimeError("no rollout() or collect() with outcomes=True has run yet")
        if not torch.is_tensor(counts) or counts.dtype != torch.int64 or counts.dim() != 2 or counts.shape[1] != L.PF_OUTCOME_SLOTS:
            raise ValueError(f"counts must be an int64 tensor of shape (G, {L.PF_OUTCOME_SLOTS}), got "
                             f"{(counts.dtype, tuple(counts.shape)) if torch.is_tensor(counts) else type(counts).__name__}")
        return [dict(zip(L.OUTCOME_SLOT_NAMES, row)) for row in counts.tolist()]

    def _reseed(self, seed, keep=()):
        """reset(seed=other): a new engine for the new seed. traj_stats' running moments outlive the old engine (its carries do not),
        and so do the state groups `keep` names (indices or slices: what a façade creates in __init__ and its reset() never rewrites)."""
        self._seed = int(seed)
        kept = [(g, self.engine.state[g].clone()) for g in keep]
        moments = self.engine.made_moments()
        self.engine.close()
        self._build(self._seed)
        self._adopt_moments(moments)
        for g, v in kept:
            self.engine.state[g] = v
        self._policy_step = 0

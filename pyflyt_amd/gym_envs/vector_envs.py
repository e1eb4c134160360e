"""Gymnasium-VectorEnv-shaped façades over the fused HIP env step.

They mirror, per lane, the reference's single-env classes (file:line under /root/reference/PyFlyt/):
  QuadXHoverVecEnv        <- gym_envs/quadx_envs/quadx_hover_env.py:10-138 (+ quadx_base_env.py)
  QuadXWaypointsVecEnv    <- gym_envs/quadx_envs/quadx_waypoints_env.py:11-204
  FixedwingWaypointsVecEnv<- gym_envs/fixedwing_envs/fixedwing_waypoints_env.py:11-190
  RocketLandingVecEnv     <- gym_envs/rocket_envs/rocket_landing_env.py (+ rocket_base_env.py)
with the same constructor keywords, action/observation layouts, reward, termination and info keys.
The reference has no vector env; the batch dimension and auto-reset follow gymnasium.vector
(num_envs, single_*_space, reset(seed=, options=), step(actions) -> 5-tuple, autoreset_mode).

Tensors are torch.float32 / torch.bool on the ROCm device and are views of buffers the kernels
write in place: copy them if you need them after the next step().

What step() costs the host (round 6): with an action tensor the env has seen before (a policy writing into a fixed buffer, an
action ring) it is one foreign call -- no tensor check, no pointer conversion, no torch kernel, no allocation, no host
synchronisation --, so a closed loop `policy(obs) -> env.step(actions)` can be captured whole in a HIP graph. `infos` is a
LazyInfos: its entries are computed from the flag words of the state when they are READ (like every other value step() returns
they describe the most recent step).
"""
from __future__ import annotations

from typing import Any

import numpy as np
import torch

from .. import _lib as L
from .._collect import ClosedLoopEnv
from ..engine import BatchEngine
from ..params import build_params
from ..spaces import Box, Dict, batch_box


class LazyInfos(dict):
    """The `infos` of a vector env step as a read-only dict whose values are computed when they are read: each is one or two
    element-wise torch kernels over the lanes' flag words, and a training loop reads them on a small fraction of its steps --
    computed eagerly they were eight kernel launches per step() against the one launch of the step itself. A key maps to a
    zero-argument function; the first read calls it and keeps the result until the env's next step() / reset(), which clears
    the cache (the values describe the MOST RECENT step: read them, or .materialize(), before stepping on if they are to be kept)."""

    __slots__ = ("_make",)

    def __init__(self, makers: dict):
        super().__init__()
        self._make = dict(makers)

    # -- the Mapping protocol over the lazy keys
    def __missing__(self, key):
        fn = self._make.get(key)
        if fn is None:
            raise KeyError(key)
        v = fn()
        dict.__setitem__(self, key, v)
        return v

    def get(self, key, default=None):
        return self[key] if key in self._make else default

    def __contains__(self, key):
        return key in self._make

    def __iter__(self):
        return iter(self._make)

    def __len__(self):
        return len(self._make)

    def keys(self):
        return self._make.keys()

    def values(self):
        return [self[k] for k in self._make]

    def items(self):
        return [(k, self[k]) for k in self._make]

    def __repr__(self):
        return "LazyInfos(" + ", ".join(f"{k!r}: " + (repr(dict.__getitem__(self, k)) if dict.__contains__(self, k) else "<lazy>") for k in self._make) + ")"

    def __setitem__(self, key, value):  # (an eager entry: kept across invalidate() only if it is set again)
        self._make[key] = lambda v=value: v
        dict.__setitem__(self, key, value)

    def invalidate(self):
        """Forget the computed values (the env calls this at every step / reset)."""
        dict.clear(self)

    def materialize(self) -> dict:
        """A plain dict of freshly computed tensors that the next step() does not touch."""
        return {k: (v.clone() if torch.is_tensor(v) else (v.materialize() if isinstance(v, LazyInfos) else v)) for k, v in self.items()}


class _VecEnvBase(ClosedLoopEnv):
    metadata = {"render_modes": [], "autoreset_mode": "next_step"}
    _vehicle = "quadx"
    _task = "hover"

    def __init__(self, num_envs: int, *, device="cuda:0", seed: int = 0, autoreset_mode: str = "next_step",
                 motor_noise: bool = True, lane_offset: int = 0, render_mode=None, **task_kwargs):
        if render_mode is not None:
            raise ValueError("rendering is out of scope for the batched GPU path (SURVEY.md section 2: Camera)")
        self.num_envs = int(num_envs)
        self.device = torch.device(device)
        self._kwargs = dict(task_kwargs)
        self._autoreset_mode = {"next_step": "next_step", "same_step": "same_step", "disabled": "off", "off": "off"}[str(autoreset_mode).lower()]
        self.metadata = dict(self.metadata, autoreset_mode=autoreset_mode)
        self._noise = "philox" if motor_noise else "off"
        self._lane_offset = int(lane_offset)
        self._seed = int(seed)
        self._build(self._seed)
        P = self.engine.params
        att = (13 if P.angle_repr else 12)
        aux = 4 if P.vehicle == L.QUADX else 6
        self.attitude_dim = att + 4 + aux
        self.single_action_space = Box(low=np.array(list(P.action_low), dtype=np.float32),
                                       high=np.array(list(P.action_high), dtype=np.float32), dtype=np.float32)
        self.action_space = batch_box(self.single_action_space, self.num_envs)
        self._make_obs_space()
        self._coerced = None  # (what the last foreign action array was converted into: kept alive until the next one)

    # ------------------------------------------------------------------ construction
    def _build(self, seed):
        P = build_params(self._vehicle, self._task, noise=self._noise, autoreset=self._autoreset_mode, seed=seed, **self._kwargs)
        self.engine = BatchEngine(P, self.num_envs, device=self.device, lane_offset=self._lane_offset)
        # what step() hands back is built ONCE per engine: views of the tensors the kernels write in place + the lazy infos
        self._ret = None
        self._infos_obj = None
        self._final_infos = None

    def _make_obs_space(self):
        self.single_observation_space = Box(low=-np.inf, high=np.inf, shape=(self.attitude_dim,), dtype=np.float32)
        self.observation_space = batch_box(self.single_observation_space, self.num_envs)

    # ------------------------------------------------------------------ gymnasium.vector API
    def reset(self, *, seed: int | None = None, options: dict | None = None):
        """Reset every env (or the subset in options['reset_mask']). A new `seed` re-keys the
        counter-based RNG (motor noise, waypoint sampling); same seed => bit-identical rollouts
        (mirrors tests/test_gym_envs.py:92-112 of the reference)."""
        mask = None if not options else options.get("reset_mask")
        if seed is not None and int(seed) != self._seed:
            if mask is not None:
                raise ValueError("cannot re-seed and partially reset in one call")
            self._reseed(seed)
        elif seed is not None and mask is None:
            # same seed: restart the event counters so that the rollout repeats exactly
            self.engine.state.zero_()
            self._policy_step = 0
        if mask is not None and not torch.is_tensor(mask):
            mask = torch.as_tensor(np.asarray(mask), dtype=torch.bool, device=self.device)
        self.engine.env_reset(mask=mask)
        self._needs_reset = False
        if self._ret is None:
            self._make_ret()
        self._infos_obj.invalidate()
        return self._obs(self.engine.obs) if self._obs_copies else self._ret[0], self._infos_obj

    def _make_ret(self):
        eng = self.engine
        infos = self._infos()
        if eng.final_obs is not None:
            # SAME_STEP (gymnasium.vector AutoresetMode.SAME_STEP): lanes that finished were re-initialised inside the
            # step, so their terminal observation AND info travel in final_obs / final_info (rows of other lanes are stale)
            fin = self._infos(eng.final_info[:, 0], eng.final_info[:, 1])
            infos._make["final_obs"] = lambda: self._obs(eng.final_obs)
            infos._make["final_info"] = lambda: fin
            infos._make["_final_info"] = lambda: eng.terminated | eng.truncated
            self._final_infos = fin
        else:
            self._final_infos = None
        self._infos_obj = infos
        self._ret = (self._obs(eng.obs), eng.reward, eng.terminated, eng.truncated, infos)

    # (FlattenWaypointEnv with a context longer than the target list pads with zeros: that observation is a fresh tensor per step)
    _obs_copies = False

    def step(self, actions):
        """gymnasium.vector.VectorEnv.step: (obs, reward, terminated, truncated, infos) for every env. The five values are the SAME
        objects every call (views of the buffers the kernel writes, and the lazy infos); nothing here synchronises with the device."""
        if self._needs_reset:
            raise RuntimeError("call reset() before step()")
        if not torch.is_tensor(actions):  # (numpy arrays, lists: one host-to-device copy per step)
            actions = self._coerced = torch.as_tensor(np.asarray(actions), dtype=torch.float32, device=self.device)
        elif actions.dtype != torch.float32 or actions.device != self.device or not actions.is_contiguous():
            actions = self._coerced = actions.to(device=self.device, dtype=torch.float32).contiguous()
        self.engine.env_step(actions)
        self._infos_obj.invalidate()
        if self._final_infos is not None:
            self._final_infos.invalidate()
        if self._obs_copies:
            r = self._ret
            return self._obs(self.engine.obs), r[1], r[2], r[3], r[4]
        return self._ret

    _pool_groups = None  # {G: [num_envs] int32}: the default segment index of every env for a list of G policies

    def _pool_args(self, policies, fused, group):
        """rollout()'s refusals for a list of policies, before anything is launched; returns the engine's group / n_groups."""
        G = len(policies)
        if not 1 <= G <= L.PF_OUTCOME_MAX_GROUPS or G > self.num_envs:
            raise ValueError(f"policy: a pool holds 1..{L.PF_OUTCOME_MAX_GROUPS} policies and at most one per env ({self.num_envs}), got {G}")
        if fused is not None and not isinstance(fused, bool):
            raise ValueError(f"fused must be None, True or False, got {fused!r}")
        if fused:
            raise ValueError("fused=True with a list of policies: the fused launch evaluates one policy; fused=None or False runs the stepwise loop with the pool launch")
        if group is None:
            groups = self._pool_groups = self._pool_groups or {}
            if G not in groups:
                from ..dist import strong_shard

                sizes = torch.tensor([strong_shard(self.num_envs, g, G).lanes for g in range(G)])
                groups[G] = torch.repeat_interleave(torch.arange(G, dtype=torch.int32), sizes).to(self.device)
            group = groups[G]
        return dict(group=group, n_groups=G)

    def rollout(self, policy, k_steps: int, store_mean: bool = False, fused=None, outcomes: bool = False, group=None):
        """`k_steps` closed-loop env steps, every action computed on the device by `policy` (a pyflyt_amd.MLPPolicy) from the
        observation the env has just returned. Returns the trajectories (obs [k, n, D] -- the engine's flat observation rows, what
        the policy reads --, reward, terminated, truncated, actions [k, n, action width]) and the infos of the LAST step (with
        store_mean the policy's means before them). The exploration noise's step index advances by k_steps per call and restarts
        with reset(seed=...).
        `fused`: None (default) = ONE launch (BatchEngine.rollout_policy) on QuadX-Hover and QuadX-Waypoints, with that launch's
        refusals, and the stepwise path on every other vehicle or task; True = the fused launch, or the library's refusal;
        False = the stepwise path, k x (pf_policy_act, pf_env_step) (BatchEngine.rollout_policy_steps), on any env -- how a
        cascaded flight mode, the generic kernel or the 8-point manifold get a closed loop. The stepwise path needs an auto-reset
        mode (ValueError). Where both exist they give the same bits.
        outcomes=True: why the episodes that finish inside the call end -- outcome [k, n] uint8 (pf_outcome_bit: 0 where no episode
        ended) and outcome_counts [1, 16] int64 on the device (episode_outcomes_dict() reads it back) come in front of the infos. One
        pf_episode_outcomes launch per step on the stepwise path; behind the fused launch, one on the final_info rows under
        SAME_STEP. Under NEXT_STEP the fused launch has nothing left to read (collect() says why): fused=None then takes the stepwise
        path, and fused=True is a ValueError.
        `policy` may be a list of 1 to 16 MLPPolicy -- checkpoints flown side by side in one batch: env i is flown by entry group[i]
        (`group`: a [num_envs] int32 tensor; default: contiguous, near-equal segments by dist.strong_shard's rule, as the dogfight's
        opponent pool uses). Only the stepwise path serves a list (fused=None takes it, fused=True is a ValueError): one
        pf_policy_pool_plan per call, then per step ONE pf_policy_act_pool, every env evaluated once by its own policy with the bits
        that policy alone would give it. outcomes=True then returns outcome_counts [G, 16], one row per policy. `group` without a
        list is a ValueError."""
        if self._needs_reset:
            raise RuntimeError("call reset() before rollout()")
        k = int(k_steps)
        if isinstance(policy, (list, tuple)):
            out = self.engine.rollout_policy_steps(list(policy), k, step_index0=self._policy_step, store_mean=store_mean, outcomes=outcomes,
                                                   **self._pool_args(policy, fused, group))
            self._after_policy_steps(k)
            return out + (self._infos_obj,)
        if group is not None:
            raise ValueError("group comes with a list of policies (which entry flies an env)")
        if self.engine._fused_policy(fused, outcomes):
            out = self.engine.rollout_policy(policy, k, step_index0=self._policy_step, store_mean=store_mean, outcomes=outcomes)
        else:
            out = self.engine.rollout_policy_steps(policy, k, step_index0=self._policy_step, store_mean=store_mean, outcomes=outcomes)
        self._after_policy_steps(k)
        return out + (self._infos_obj,)

    def _after_policy_steps(self, k):
        """What rollout() and collect() do once their k steps are enqueued: the noise's step index moves on, the infos are stale.
        (step() invalidates the infos itself: it is one foreign call and nothing else, and it leaves the step index alone.)"""
        self._policy_step = (self._policy_step + k) & 0xFFFFFFFF
        self._infos_obj.invalidate()
        if self._final_infos is not None:
            self._final_infos.invalidate()

    def collect(self, policy, value_fn, k_steps: int, gamma: float = 0.99, lam: float = 0.95, stats: bool = False, normalize_reward: bool = False,
                fused=None, outcomes: bool = False):
        """One PPO batch from `k_steps` closed-loop env steps: the closed loop of rollout() (`fused` as there: one launch on
        QuadX-Hover / QuadX-Waypoints, the stepwise path on every other env), the caller's value network, and
        pf_gae (BatchEngine.gae) -- obs -> policy -> env -> batch ready for the loss, without a host synchronisation.
        `value_fn`: any torch callable from a float32 [M, D] tensor to [M] or [M, 1] (float32); it is called under torch.no_grad(),
        once on all k + 1 observation rows and, under SAME_STEP auto-reset, once more on the final_obs trajectory.
        Returns a dict: obs [k, n, D] the policy's inputs, actions, mean, logp (None for a policy without log_std), values [k, n],
        advantages, returns, valid [k, n] bool (False on the steps that only reset a lane under NEXT_STEP: mask the losses with it),
        reward, terminated, truncated, last_value [n] (the value of the observation after the last step) and the infos of the last
        step. obs is a view of the engine's [k + 1, n, D] buffer: obs[s + 1] is the very row the env wrote as step s's next
        observation. The tensors belong to the engine and are overwritten by the next collect() with the same
        k_steps. The exploration noise's step index advances as in rollout().
        stats=True runs pf_traj_stats (BatchEngine.traj_stats) on the same trajectory before pf_gae and adds episode_return,
        episode_length [k, n] (the finished episode's return and length where an episode ended in a valid step, 0 elsewhere) and
        episode_summary ([8] float64 on the device; episode_summary_dict() reads it back); it updates the running moments behind
        obs_rms (the columns of the policy's inputs) and ret_rms (the discounted return, with this call's gamma) over the valid steps.
        normalize_reward=True implies stats, hands pf_gae reward / sqrt(ret_rms.var + 1e-8) with the moments AFTER this batch's
        update, and adds it as reward_scaled; reward stays raw. The episode accounting is carried from one collect(stats=True) to the
        next and sees only their steps: a step(), rollout() or collect() without stats in between advances the env behind its back,
        and the first episode_return / episode_length after it would lack those steps -- reset() the env before switching.
        outcomes=True adds outcome [k, n] uint8 (pf_outcome_bit of every episode that ended: ended, terminated, collision, out of
        bounds, env_complete, nonfinite) and outcome_counts [1, 16] int64 on the device, the counts of THIS call's episodes by slot
        (episode_outcomes_dict() reads them back by name; slot 8 is the sum of num_targets_reached on the waypoint envs). On the
        stepwise path each step enqueues one pf_episode_outcomes launch behind pf_env_step. The fused launch keeps the flags in
        registers and resets lanes inside the launch: under SAME_STEP its final_info rows hold every ended episode's words and one
        call behind the launch reads them; under NEXT_STEP nothing holds them, so fused=None runs the stepwise loop (the same bits,
        at the stepwise loop's price) and fused=True with outcomes=True is a ValueError.
        A list of policies is refused (ValueError): a batch has one behaviour policy; rollout() flies a list."""
        if isinstance(policy, (list, tuple)):
            raise ValueError("collect() takes one policy, not a list: a batch has one behaviour policy (rollout() flies a list of policies side by side)")
        stats = self._collect_args(policy, value_fn, gamma, lam, stats, normalize_reward, outcomes)
        eng, k = self.engine, int(k_steps)
        if not eng._fused_policy(fused, outcomes):  # (refused before the flags are read or anything is launched)
            eng._check_stepwise()
        episode_start = None
        if eng.params.autoreset == L.AUTORESET_NEXT_STEP:
            # lanes whose last step ended an episode: the launch's first step only resets them (read before the launch rewrites the flags)
            episode_start = (eng.flags() & (L.F_TERMINATED | L.F_TRUNCATED)) != 0
        t = eng.collect_rollout(policy, k, step_index0=self._policy_step, fused=fused, outcomes=outcomes)
        self._after_policy_steps(k)
        return self._collect_batch(t, policy, value_fn, gamma, lam, stats, normalize_reward, self._infos_obj, episode_start=episode_start, outcomes=outcomes)

    def sample_actions(self, step_index: int = 0):
        """Device-side uniform sample of the action box (the role of action_space.sample())."""
        out = torch.empty(self.num_envs, 4, dtype=torch.float32, device=self.device)
        return self.engine.sample_actions(out, step_index)

    # ------------------------------------------------------------------ helpers
    def _obs(self, buf):
        return buf

    def _infos(self, flags=None, n_left=None) -> LazyInfos:
        f = self.engine.flags() if flags is None else flags  # (a view of the state's int group: read when an entry is)
        return LazyInfos({
            "out_of_bounds": lambda: (f & L.F_INFO_OOB) != 0,      # quadx_base_env.py:266
            "collision": lambda: (f & L.F_INFO_COLLISION) != 0,    # quadx_base_env.py:260
            "env_complete": lambda: (f & L.F_INFO_COMPLETE) != 0,  # quadx_waypoints_env.py:203
            "nonfinite": lambda: (f & L.F_NONFINITE) != 0,         # NaN/Inf guard (not in the reference, which carries NaNs on silently)
        })

    @property
    def step_count(self):
        return self.engine.ints()[:, 0]


class QuadXHoverVecEnv(_VecEnvBase):
    """PyFlyt/QuadX-Hover-v4, batched. Keywords as quadx_hover_env.py:32-41."""
    _vehicle, _task = "quadx", "hover"

    def __init__(self, num_envs: int, *, sparse_reward: bool = False, flight_mode: int = 0, flight_dome_size: float = 3.0,
                 max_duration_seconds: float = 10.0, angle_representation: str = "quaternion", agent_hz: int = 40, **kw):
        super().__init__(num_envs, sparse_reward=sparse_reward, flight_mode=flight_mode, flight_dome_size=flight_dome_size,
                         max_duration_seconds=max_duration_seconds, angle_representation=angle_representation,
                         agent_hz=agent_hz, **kw)


class _WaypointsMixin:
    def _make_obs_space(self):
        nt = self.engine.params.num_targets
        dome = self.engine.params.dome
        self.num_targets = nt
        tw = self.target_width = 4 if self.engine.params.use_yaw_targets else 3  # quadx_waypoints_env.py:99
        if self._flatten:
            width = self.attitude_dim + tw * self._context_length
            self.single_observation_space = Box(low=-np.inf, high=np.inf, shape=(width,), dtype=np.float32)
            self.observation_space = batch_box(self.single_observation_space, self.num_envs)
        else:
            self.single_observation_space = Dict({
                "attitude": Box(low=-np.inf, high=np.inf, shape=(self.attitude_dim,), dtype=np.float32),
                "target_deltas": Box(low=-2 * dome, high=2 * dome, shape=(nt, tw), dtype=np.float32),
            })
            self.observation_space = Dict({
                "attitude": batch_box(self.single_observation_space["attitude"], self.num_envs),
                "target_deltas": batch_box(self.single_observation_space["target_deltas"], self.num_envs),
            })

    def _obs(self, buf):
        a, tw = self.attitude_dim, self.target_width
        if self._flatten:  # gym_envs/utils/flatten_waypoint_env.py:42-62
            ctx = self._context_length
            have = min(ctx, self.num_targets)
            if have == ctx:
                return buf[:, : a + tw * ctx]
            pad = torch.zeros(buf.shape[0], tw * (ctx - have), dtype=buf.dtype, device=buf.device)
            return torch.cat([buf[:, : a + tw * have], pad], dim=1)
        # the reference's variable-length Sequence becomes a fixed [num_targets, 3] block whose rows
        # past the remaining targets are zero (flatten_waypoint_env.py:49-56 padding convention)
        return {"attitude": buf[:, :a], "target_deltas": buf[:, a:].view(-1, self.num_targets, tw)}

    def _infos(self, flags=None, n_left=None):
        infos = super()._infos(flags)
        if n_left is None:
            n_left = self.engine.ints()[:, 3]
        infos._make["num_targets_reached"] = lambda: self.num_targets - n_left  # quadx_waypoints_env.py:204
        return infos

    @property
    def _obs_copies(self):
        return self._flatten and self._context_length > self.num_targets


class QuadXWaypointsVecEnv(_WaypointsMixin, _VecEnvBase):
    """PyFlyt/QuadX-Waypoints-v4, batched. Keywords as quadx_waypoints_env.py:36-49, incl. `use_yaw_targets` /
    `goal_reach_angle` (target deltas 4 wide: body-frame delta + wrapped yaw error; a waypoint counts only when
    both gates hold). flatten=True returns FlattenWaypointEnv-style rows [attitude, ctx deltas]."""
    _vehicle, _task = "quadx", "waypoints"

    def __init__(self, num_envs: int, *, sparse_reward: bool = False, num_targets: int = 4, use_yaw_targets: bool = False,
                 goal_reach_distance: float = 0.2, goal_reach_angle: float = 0.1, flight_mode: int = 0,
                 flight_dome_size: float = 5.0, max_duration_seconds: float = 10.0, angle_representation: str = "quaternion",
                 agent_hz: int = 30, flatten: bool = False, context_length: int = 2, **kw):
        self._flatten, self._context_length = bool(flatten), int(context_length)
        super().__init__(num_envs, sparse_reward=sparse_reward, num_targets=num_targets, goal_reach_distance=goal_reach_distance,
                         use_yaw_targets=use_yaw_targets, goal_reach_angle=goal_reach_angle, flight_mode=flight_mode, flight_dome_size=flight_dome_size, max_duration_seconds=max_duration_seconds,
                         angle_representation=angle_representation, agent_hz=agent_hz, **kw)


class FixedwingWaypointsVecEnv(_WaypointsMixin, _VecEnvBase):
    """PyFlyt/Fixedwing-Waypoints-v4, batched. Keywords as fixedwing_waypoints_env.py:36-47."""
    _vehicle, _task = "fixedwing", "waypoints"

    def __init__(self, num_envs: int, *, sparse_reward: bool = False, num_targets: int = 4, goal_reach_distance: float = 2.0,
                 flight_mode: int = 0, flight_dome_size: float = 100.0, max_duration_seconds: float = 120.0,
                 angle_representation: str = "quaternion", agent_hz: int = 30, flatten: bool = False,
                 context_length: int = 2, **kw):
        self._flatten, self._context_length = bool(flatten), int(context_length)
        super().__init__(num_envs, sparse_reward=sparse_reward, num_targets=num_targets, goal_reach_distance=goal_reach_distance,
                         flight_mode=flight_mode, flight_dome_size=flight_dome_size, max_duration_seconds=max_duration_seconds,
                         angle_representation=angle_representation, agent_hz=agent_hz, **kw)


class RocketLandingVecEnv(_VecEnvBase):
    """PyFlyt/Rocket-Landing-v4, batched: gym_envs/rocket_envs/rocket_landing_env.py (+ rocket_base_env.py). Keywords as
    rocket_landing_env.py:37-46. Actions [n, 7]: finlet x, finlet y, finlet roll, ignition, throttle, gimbal 1, gimbal 2 in
    low (-1, -1, -1, 0, 0, -1, -1), high 1. Observation [n, 30] (quaternion) or [n, 29] (euler): ang_vel, attitude, lin_vel,
    lin_pos, action (7), aux (9), landing-pad contact -- the pad value lags one Aviary step, as the reference's does.
    reset(options=...): None (what gymnasium.make passes) turns on randomize_drop and accelerate_drop, a dict each key it holds
    (options={}: neither); auto-resets reuse the options of the last reset(). A different set rebuilds the context, so it cannot
    come with a reset_mask; a dict holding only reset_mask keeps the current set. (The reference keeps a randomized spawn in
    self.start_pos, so its next reset with options={} starts there; here such a reset starts from `start_pos`.)
    Not in make_vec / make yet: "PyFlyt/Rocket-Landing-v4" stays the unknown-id probe of the existing API tests; registering it
    is a one-line follow-up together with a new probe id."""
    _vehicle, _task = "rocket", "rocket_landing"
    _LOW = (-1.0, -1.0, -1.0, 0.0, 0.0, -1.0, -1.0)  # rocket_base_env.py:95-119

    def __init__(self, num_envs: int, *, sparse_reward: bool = False, ceiling: float = 500.0, max_displacement: float = 200.0,
                 max_duration_seconds: float = 30.0, angle_representation: str = "quaternion", agent_hz: int = 40, **kw):
        super().__init__(num_envs, sparse_reward=sparse_reward, ceiling=ceiling, max_displacement=max_displacement,
                         max_duration_seconds=max_duration_seconds, angle_representation=angle_representation, agent_hz=agent_hz,
                         reset_options=L.RL_RANDOMIZE_DROP | L.RL_ACCELERATE_DROP, **kw)
        self.single_action_space = Box(low=np.array(self._LOW, dtype=np.float32), high=np.ones(7, dtype=np.float32), dtype=np.float32)
        self.action_space = batch_box(self.single_action_space, self.num_envs)

    def _make_obs_space(self):
        P = self.engine.params
        self.attitude_dim = (13 if P.angle_repr else 12) + 7 + 9  # rocket_base_env.py:77-126 (combined_space)
        low = np.full(self.attitude_dim + 1, -np.inf, dtype=np.float32)
        high = np.full(self.attitude_dim + 1, np.inf, dtype=np.float32)
        low[-1], high[-1] = 0.0, 1.0  # the pad contact (rocket_landing_env.py:69-73)
        self.single_observation_space = Box(low=low, high=high, dtype=np.float32)
        self.observation_space = batch_box(self.single_observation_space, self.num_envs)

    def reset(self, *, seed: int | None = None, options: dict | None = None):
        if options is None:
            bits = L.RL_RANDOMIZE_DROP | L.RL_ACCELERATE_DROP
        elif not ({"randomize_drop", "accelerate_drop"} & set(options)) and "reset_mask" in options:
            bits = self._kwargs["reset_options"]
        else:
            bits = (L.RL_RANDOMIZE_DROP if options.get("randomize_drop", False) else 0) | \
                   (L.RL_ACCELERATE_DROP if options.get("accelerate_drop", False) else 0)
        if bits != self._kwargs["reset_options"]:
            if options is not None and options.get("reset_mask") is not None:
                raise ValueError("cannot change the reset options in a partial reset")
            self._kwargs["reset_options"] = bits
            self._seed = self._seed if seed is None else int(seed)
            self.engine.close()
            self._build(self._seed)
            self._policy_step = 0
        return super().reset(seed=seed, options=options)

    def sample_actions(self, step_index: int = 0):
        """Device-side uniform sample of the seven-wide action box (the role of action_space.sample())."""
        out = torch.empty(self.num_envs, 7, dtype=torch.float32, device=self.device)
        return self.engine.sample_actions(out, step_index)

    def _infos(self, flags=None, n_left=None) -> LazyInfos:
        f = self.engine.flags() if flags is None else flags
        return LazyInfos({
            "out_of_bounds": lambda: (f & L.F_INFO_OOB) != 0,          # rocket_base_env.py:293-299
            "fatal_collision": lambda: (f & L.F_INFO_COLLISION) != 0,  # rocket_base_env.py:287-291, rocket_landing_env.py:228-232
            "env_complete": lambda: (f & L.F_INFO_COMPLETE) != 0,      # rocket_landing_env.py:234-242
            "nonfinite": lambda: (f & L.F_NONFINITE) != 0,
        })


_REGISTRY = {
    # ids as registered by the reference, gym_envs/__init__.py:8-43
    "PyFlyt/QuadX-Hover-v4": QuadXHoverVecEnv,
    "PyFlyt/QuadX-Waypoints-v4": QuadXWaypointsVecEnv,
    "PyFlyt/Fixedwing-Waypoints-v4": FixedwingWaypointsVecEnv,
}


def make_vec(env_id: str, num_envs: int, devices=None, **kwargs):
    """The batched counterpart of `gymnasium.make_vec(id, num_envs=...)` for the supported ids. devices=[...]: the num_envs lanes cut
    into one vector env per device, behind a ShardedVecEnv (gym_envs/sharded.py)."""
    if env_id not in _REGISTRY:
        raise KeyError(f"{env_id!r} is not on the batched hot path; available: {sorted(_REGISTRY)}")
    if devices is not None:
        from .sharded import ShardedVecEnv

        return ShardedVecEnv(_REGISTRY[env_id], num_envs, devices, **kwargs)
    return _REGISTRY[env_id](num_envs, **kwargs)


class SingleEnv:
    """One environment with the reference's single-env calling convention -- what
    `gymnasium.make("PyFlyt/QuadX-Hover-v4")` hands back (numpy observations, Python scalars, no
    auto-reset; quadx_base_env.py:128-301) -- on top of a 1-lane batch. For existing scripts and tests;
    throughput comes from `make_vec`."""

    def __init__(self, env_id: str, **kwargs):
        kwargs.pop("autoreset_mode", None)
        self.vec = make_vec(env_id, 1, autoreset_mode="disabled", **kwargs)
        self.observation_space = self.vec.single_observation_space
        self.action_space = self.vec.single_action_space
        self.metadata = dict(self.vec.metadata)
        self.unwrapped = self

    @staticmethod
    def _np(x):
        if isinstance(x, dict):
            return {k: SingleEnv._np(v) for k, v in x.items()}
        return x[0].detach().cpu().numpy()

    def _info(self, infos):
        return {k: (SingleEnv._np(v) if torch.is_tensor(v) or isinstance(v, dict) else v) for k, v in infos.items()}

    def reset(self, *, seed: int | None = None, options: dict | None = None):
        obs, infos = self.vec.reset(seed=seed)
        return self._np(obs), {k: (bool(v) if getattr(v, "dtype", None) == np.bool_ else v) for k, v in self._info(infos).items()}

    def step(self, action):
        a = torch.as_tensor(np.asarray(action, dtype=np.float32).reshape(1, 4), device=self.vec.device)
        obs, rew, term, trunc, infos = self.vec.step(a)
        info = {k: (bool(v) if getattr(v, "dtype", None) == np.bool_ else v) for k, v in self._info(infos).items()}
        return self._np(obs), float(rew[0]), bool(term[0]), bool(trunc[0]), info

    def close(self):
        self.vec.close()


def make(env_id: str, **kwargs) -> SingleEnv:
    """The counterpart of `gymnasium.make(id, **kwargs)` for the supported ids."""
    return SingleEnv(env_id, **kwargs)

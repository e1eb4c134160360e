"""The training operations of a BatchEngine -- pf_gae, pf_traj_stats / pf_traj_stats_masked, pf_ppo_loss, pf_mlp_forward / pf_mlp_backward, pf_adam_step --
and the plumbing they share with the env level in engine.py: the tensor check bound to the engine's device, the launch wrapper and
the state an engine makes at first use. A base class without __init__: everything here works on an engine that has only `n`,
`device`, `params` and `_ctx` (and `obs_dim` for traj_stats), which is how the CPU tests reach the refusals.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _checks as K
from . import _lib as L


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


try:  # the raw handle of torch's current stream without building a torch.cuda.Stream object (0.2 us against 1.5 us per call)
    _raw_stream = torch._C._cuda_getCurrentRawStream
except AttributeError:  # pragma: no cover
    def _raw_stream(index):
        return torch.cuda.current_stream(index).cuda_stream


class TrainOps:
    # state made at first use, by _lazy only: None until then (class attributes, so an engine made without __init__ has them too)
    _traj = None      # dict: the trajectory tensors rollout(), rollout_policy() and rollout_policy_steps() share, for the last k
    _ctraj = None     # dict: collect_rollout()'s trajectory tensors (observations in one [k + 1, n, D] buffer), for the last k
    _gae_out = None   # dict: gae()'s advantages / returns / logp / valid, for the last k
    _ts = None        # dict: traj_stats()'s per-lane carries, summary, the two running moment blocks, the per-step outputs of the last k
    _ppo_out = None   # dict: ppo_loss()'s gradients for the last (M, A), stats, and the count of calls
    _mlp_fwd = None   # {(rows, out_dim): mlp_forward()'s output}
    _mlp_bwd = None   # {(rows, layer shapes): mlp_backward()'s gradients, pointer arrays and workspace}
    _ppo_grad = None  # {(rows, both networks' layer shapes): ppo_grad()'s gradients, argument block and workspace}; "stats": its [16] block
    _ppo_shard = None  # {(rows, both networks' layer shapes): ppo_grad_shard()'s flat gradients, block, argument block and workspace}; the sums' and the combine's outputs
    _adam = None      # {addresses: adam_step()'s filled argument block}, the 64 most recent
    _adam_ws = None   # {total elements: adam_step()'s workspace}
    _world_done = None  # [n] uint8: world_sync's latch as the world rollouts keep it (BatchEngine.world_done)
    _world_out = None   # dict: world_sync()'s valid / reset mask when the caller passes none
    _wtraj = None     # dict: rollout_policy_worlds()'s trajectory tensors, for the last k
    _wctraj = None    # dict: collect_rollout_worlds()'s (observations in one [k + 1, n, D] buffer), for the last k
    _opp_act = None   # [n, action width] float32: rollout_policy_worlds()'s opponent actions before the merge
    _world_outcome = None  # [n] uint8: episode_outcomes' world latch as the world rollouts keep it (BatchEngine.world_outcome)
    _oc_last = None   # [G, 16] int64: the outcome counts of the last closed loop with outcomes=True

    def _lazy(self, name, make, keep=None):
        """self.<name> of the list above: made by make() at first use, and again when keep(it) is false (tensors of another size)."""
        v = getattr(self, name)
        if v is None or (keep is not None and not keep(v)):
            v = make()
            setattr(self, name, v)
        return v

    # ------------------------------------------------------------------ helpers
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _launch(self, fn, *args):
        """fn(ctx, *args, stream) on the engine's device and torch's current stream; a refusal raises with the context's message."""
        with torch.cuda.device(self.device):
            L.check(fn(self._ctx, *args, self._stream()), self._ctx)

    def _traj_args(self, reward, terminated, truncated):
        """What gae and traj_stats ask of a trajectory before anything else: reward [k, n] float32 with k >= 1, terminated and
        truncated [k, n] bool / uint8. Returns k."""
        K.ranked(reward, "reward", f"{{name}} must be a float32 tensor of shape (k, {self.n})", 2)
        k = int(reward.shape[0])
        if k < 1:
            raise ValueError("reward must hold at least one step")
        K.tensor(self.device, reward, "reward", (k, self.n))
        for name, x in (("terminated", terminated), ("truncated", truncated)):
            if x is None:
                raise ValueError(f"{name} is required")
            K.tensor(self.device, x, name, (k, self.n), K.FLAGS)
        return k

    def _episode_start(self, episode_start):
        """The rest of that preamble, which comes after the scalars in both: episode_start [n] bool / uint8, NEXT_STEP only."""
        if self.params.autoreset != L.AUTORESET_NEXT_STEP and episode_start is not None:
            raise ValueError("episode_start must be None outside NEXT_STEP auto-reset (no other mode has reset steps)")
        K.tensor(self.device, episode_start, "episode_start", (self.n,), K.FLAGS)

    # ------------------------------------------------------------------ advantages and episode statistics
    def gae(self, reward, terminated, truncated, values, gamma: float = 0.99, lam: float = 0.95, final_values=None, episode_start=None,
            actions=None, mean=None, log_std=None):
        """pf_gae: which steps of a trajectory are real transitions, their advantages and returns by generalised advantage
        estimation, and the log-probabilities of the actions (include/pyflyt_amd.h has the semantics). reward / terminated /
        truncated [k, n] as a rollout wrote them; values [k + 1, n]: row s the value of the observation the policy saw at step s,
        row k that of the last observation; final_values [k, n]: the value of final_obs, SAME_STEP only (and required there);
        episode_start [n]: NEXT_STEP only, lanes that were waiting for their reset when the rollout began; actions, mean [k, n, A]
        and log_std [A] together, or none of them (then logp is None). Returns (advantages [k, n], returns [k, n], logp [k, n] or
        None, valid [k, n] bool): tensors the engine owns, overwritten by the next call with the same k."""
        k, A = self._traj_args(reward, terminated, truncated), self.action_dim
        if values is None:
            raise ValueError("values is required")
        K.tensor(self.device, values, "values", (k + 1, self.n))
        K.unit_interval(gamma, "gamma")
        K.unit_interval(lam, "lam")
        same = self.params.autoreset == L.AUTORESET_SAME_STEP
        if same and final_values is None:
            raise ValueError("final_values is required under SAME_STEP auto-reset (the value of the terminal observation in final_obs)")
        if not same and final_values is not None:
            raise ValueError("final_values must be None outside SAME_STEP auto-reset (there is no final_obs)")
        self._episode_start(episode_start)
        K.tensor(self.device, final_values, "final_values", (k, self.n))
        given = [x is not None for x in (actions, mean, log_std)]
        if any(given) and not all(given):
            raise ValueError("actions, mean and log_std come together or not at all")
        K.tensor(self.device, actions, "actions", (k, self.n, A))
        K.tensor(self.device, mean, "mean", (k, self.n, A))
        K.tensor(self.device, log_std, "log_std", (A,))
        o = self._lazy("_gae_out", lambda: dict(k=k, valid=torch.empty(k, self.n, dtype=torch.bool, device=self.device),
                                                **{name: torch.empty(k, self.n, dtype=torch.float32, device=self.device) for name in ("advantages", "returns", "logp")}),
                       keep=lambda o: o["k"] == k)
        a = L.PfGae()
        a.gamma = float(gamma)
        setattr(a, "lambda", float(lam))
        a.reward, a.terminated, a.truncated, a.values = _ptr(reward), _ptr(terminated), _ptr(truncated), _ptr(values)
        a.final_values, a.episode_start = _ptr(final_values), _ptr(episode_start)
        a.actions, a.mean, a.log_std = _ptr(actions), _ptr(mean), _ptr(log_std)
        a.advantages, a.returns, a.valid_out = _ptr(o["advantages"]), _ptr(o["returns"]), _ptr(o["valid"])
        a.logp_out = _ptr(o["logp"]) if all(given) else None
        self._launch(self.lib.pf_gae, C.byref(a), k)
        return o["advantages"], o["returns"], (o["logp"] if all(given) else None), o["valid"]

    def _traj_state(self):
        """What traj_stats keeps between calls, made at its first use: the per-lane carries, summary and the two running moment blocks."""
        def make(zeros=torch.zeros, f32=torch.float32, f64=torch.float64):
            return dict(carry_return=zeros(self.n, dtype=f32, device=self.device), carry_length=zeros(self.n, dtype=torch.int32, device=self.device),
                        carry_disc=zeros(self.n, dtype=f32, device=self.device), summary=zeros(8, dtype=f64, device=self.device),
                        obs_moments=zeros(1 + 2 * self.obs_dim, dtype=f64, device=self.device), ret_moments=zeros(3, dtype=f64, device=self.device), k=0)
        return self._ts or self._lazy("_ts", make)

    @property
    def obs_moments(self):
        """[1 + 2 D] float64 (count, mean[D], M2[D]): the running moments of the observation columns (traj_stats with obs=)."""
        return self._traj_state()["obs_moments"]

    @property
    def ret_moments(self):
        """[3] float64 (count, mean, M2): the running moments of the discounted return G (traj_stats)."""
        return self._traj_state()["ret_moments"]

    def made_moments(self):
        """(obs_moments, ret_moments) if traj_stats' state has been made, else None -- without making it: what a re-seeded env carries
        over to its next engine."""
        return None if self._ts is None else (self._ts["obs_moments"], self._ts["ret_moments"])

    def reset_moments(self):
        """Zero the running moments of traj_stats (the empty state). The carries of the open episodes stay."""
        ts = self._traj_state()
        ts["obs_moments"].zero_()
        ts["ret_moments"].zero_()

    def traj_stats(self, reward, terminated, truncated, gamma: float = 0.99, episode_start=None, obs=None, store_steps: bool = True, valid=None):
        """pf_traj_stats: the return and length of every episode that finished inside a trajectory, and the running moments of a
        reward and an observation normaliser (include/pyflyt_amd.h has the semantics). reward / terminated / truncated [k, n] as a
        rollout wrote them; episode_start [n]: NEXT_STEP only, as for gae(); obs [k, n, D]: the observations the policy saw (collect's
        obs), or None for no observation moments; store_steps=False skips the two per-step outputs. valid [k, n] bool / uint8: the
        steps that are transitions, given instead of derived from the auto-reset mode -- the call is then pf_traj_stats_masked (the
        multi-agent rollouts' valid, pf_world_sync's; flags, reward and observation of the other steps are ignored), in any mode,
        and episode_start must be None. The engine owns the per-lane
        carries (a trajectory may be split over calls; env_reset zeroes the lanes it resets), summary and the running moments
        (self.obs_moments, self.ret_moments; reset_moments() empties them). The carries describe the lanes' open episodes only if
        EVERY env step since the last reset goes through traj_stats, in order: steps taken by env_step, rollout or a collect without
        stats in between are not seen, and the next finished episode's return and length would miss them -- reset the lanes (or
        zero the carries) before mixing the two. Returns (episode_return [k, n], episode_length [k, n]
        int32 -- both None without store_steps --, summary [8] float64): overwritten by the next call with the same k."""
        k = self._traj_args(reward, terminated, truncated)
        K.unit_interval(gamma, "gamma")
        if valid is not None and episode_start is not None:
            raise ValueError("valid and episode_start do not come together (valid says which steps are transitions; there is no reset step to derive)")
        self._episode_start(episode_start)
        K.tensor(self.device, valid, "valid", (k, self.n), K.FLAGS)
        if obs is not None:
            K.tensor(self.device, obs, "obs", (k, self.n, self.obs_dim), required=f"{{name}} must be a float32 tensor of shape (k, {self.n}, D)")
        ts = self._traj_state()
        if store_steps and ts["k"] != k:
            ts.update(k=k, episode_return=torch.empty(k, self.n, dtype=torch.float32, device=self.device),
                      episode_length=torch.empty(k, self.n, dtype=torch.int32, device=self.device))
        a = L.PfTrajStats() if valid is None else L.PfTrajStatsMasked()
        a.gamma = float(gamma)
        a.reward, a.terminated, a.truncated = _ptr(reward), _ptr(terminated), _ptr(truncated)
        if valid is None:
            a.episode_start = _ptr(episode_start)
        else:
            a.valid = _ptr(valid)
        a.obs, a.obs_moments = _ptr(obs), (_ptr(ts["obs_moments"]) if obs is not None else None)
        a.carry_return, a.carry_length, a.carry_disc = _ptr(ts["carry_return"]), _ptr(ts["carry_length"]), _ptr(ts["carry_disc"])
        a.ep_return_out = _ptr(ts["episode_return"]) if store_steps else None
        a.ep_length_out = _ptr(ts["episode_length"]) if store_steps else None
        a.summary, a.ret_moments = _ptr(ts["summary"]), _ptr(ts["ret_moments"])
        self._launch(self.lib.pf_traj_stats if valid is None else self.lib.pf_traj_stats_masked, C.byref(a), k)
        return (ts["episode_return"] if store_steps else None), (ts["episode_length"] if store_steps else None), ts["summary"]

    # ------------------------------------------------------------------ why episodes end
    def _outcome_shape(self, k, info_given, n_groups, agents_per_world, has_reset, has_latch):
        """pf_episode_outcomes' refusals that need no tensor, in the library's order; returns A."""
        if self.params.task == L.TASK_NONE:
            raise ValueError("episode_outcomes needs an engine with an env task")
        if not info_given and k != 1:
            raise ValueError(f"info is required for a trajectory of k > 1 steps (the live state holds the words of one step), got k = {k}")
        if isinstance(n_groups, bool) or not isinstance(n_groups, int) or not 1 <= n_groups <= L.PF_OUTCOME_MAX_GROUPS:
            raise ValueError(f"n_groups must be an int in 1..{L.PF_OUTCOME_MAX_GROUPS}, got {n_groups!r}")
        A = int(agents_per_world)
        if not 1 <= A <= 64 or self.n % A != 0:
            raise ValueError(f"agents_per_world must be in 1..64 and divide the lane count {self.n}, got {agents_per_world}")
        if A > 1 and k != 1:
            raise ValueError(f"the world form (agents_per_world > 1) runs once per step: k must be 1, got {k}")
        if A > 1 and not (has_reset and has_latch):
            raise ValueError("world_reset (world_sync's reset mask of this step) and world_latch are required with agents_per_world > 1")
        if A == 1 and has_reset:
            raise ValueError("world_reset must be None with agents_per_world == 1 (there are no worlds to tally)")
        return A

    def episode_outcomes(self, terminated, truncated, counts, valid=None, info=None, group=None, n_groups: int = 1, agents_per_world: int = 1,
                         world_reset=None, world_latch=None, outcome_out=None):
        """pf_episode_outcomes: why the episodes of a trajectory ended, counted per group of lanes into `counts` ([n_groups, 16] int64,
        ADDED to in place; include/pyflyt_amd.h has the slots and the bits). terminated / truncated [k, n] bool / uint8 (or [n]: one
        step) as a rollout wrote them; valid [k, n] or None: whose ended episodes are counted (pf_world_sync's); info [k, n, 2] int32
        in final_info's layout, or None = the words of the engine's state as the env step left it (one step only); group [n] int32
        in 0..n_groups-1 or None; outcome_out [k, n] uint8 or None: the byte of every ended episode. With agents_per_world > 1 (one
        step): world_reset [n], this step's reset mask of world_sync, and world_latch [n] uint8, the caller's (self.world_outcome is
        the world rollouts'). One launch, nothing synchronises. Returns counts."""
        K.ranked(terminated, "terminated", f"{{name}} is required: a bool / uint8 tensor of shape (k, {self.n}) or ({self.n},)")
        k = 1 if terminated.dim() == 1 else int(terminated.shape[0])
        if k < 1:
            raise ValueError("terminated must hold at least one step")
        A = self._outcome_shape(k, info is not None, n_groups, agents_per_world, world_reset is not None, world_latch is not None)
        rows = ((k, self.n), (self.n,)) if k == 1 else ((k, self.n),)
        need = "{name} is required: a tensor of shape {shape}"
        K.tensor(self.device, terminated, "terminated", rows, K.FLAGS, required=need)
        K.tensor(self.device, truncated, "truncated", rows, K.FLAGS, required=need)
        K.tensor(self.device, counts, "counts", (n_groups, L.PF_OUTCOME_SLOTS), torch.int64, required=need)
        K.tensor(self.device, valid, "valid", rows, K.FLAGS)
        K.tensor(self.device, info, "info", ((k, self.n, 2), (self.n, 2)) if k == 1 else ((k, self.n, 2),), torch.int32)
        K.tensor(self.device, group, "group", (self.n,), torch.int32)
        K.tensor(self.device, world_reset, "world_reset", (self.n,), K.FLAGS)
        K.tensor(self.device, world_latch, "world_latch", (self.n,), torch.uint8)
        K.tensor(self.device, outcome_out, "outcome_out", rows, torch.uint8)
        a = L.PfOutcome()
        a.terminated, a.truncated, a.valid, a.info = _ptr(terminated), _ptr(truncated), _ptr(valid), _ptr(info)
        a.state = _ptr(self.state) if info is None else None
        a.group, a.n_groups, a.world_reset, a.world_latch = _ptr(group), n_groups, _ptr(world_reset), _ptr(world_latch)
        a.outcome_out, a.counts = _ptr(outcome_out), _ptr(counts)
        self._launch(self.lib.pf_episode_outcomes, C.byref(a), k, A)
        return counts

    @property
    def world_outcome(self):
        """[n] uint8, made at first use: episode_outcomes' world latch as the world rollouts keep it, beside world_done -- the byte
        of the episode each lane last ended. Nothing ever clears it: a world is tallied only after every one of its lanes has ended
        again, and a world reset from outside is not tallied."""
        return self._lazy("_world_outcome", lambda: torch.zeros(self.n, dtype=torch.uint8, device=self.device))

    def _outcome_block(self, t, k, group, n_groups):
        """What a closed loop with outcomes=True writes, kept with its trajectory tensors `t`: t["outcome"] [k, n] uint8 and
        t["outcome_counts"] [n_groups, 16] int64, zeroed here -- the counts are of this call's episodes. Returns the filled
        pf_outcome_args block but for the per-step pointers."""
        K.tensor(self.device, group, "group", (self.n,), torch.int32)
        if t.get("outcome") is None:
            t["outcome"] = torch.empty(k, self.n, dtype=torch.uint8, device=self.device)
        c = t.get("outcome_counts")
        if c is None or c.shape[0] != n_groups:
            c = t["outcome_counts"] = torch.empty(n_groups, L.PF_OUTCOME_SLOTS, dtype=torch.int64, device=self.device)
        c.zero_()
        self._oc_last = c
        a = L.PfOutcome()
        a.group, a.n_groups, a.counts = _ptr(group), n_groups, _ptr(c)
        a.state = _ptr(self.state)
        return a

    # ------------------------------------------------------------------ the loss
    def _ppo_tensors(self, table):
        """What ppo_loss and ppo_grad ask of the tensors they read, a table of (name, tensor, admitted shapes, dtypes) in the order
        of the refusals: every one is required, but for `valid`."""
        for name, t, shapes, dtypes in table:
            if name != "valid" or t is not None:
                K.tensor(self.device, t, name, shapes, dtypes, required="{name} is required: a tensor of shape {shape}")

    @staticmethod
    def _ppo_coefficients(clip, vf_coef, ent_coef, normalize_advantage):
        """What ppo_loss and ppo_grad ask of the loss's coefficients."""
        for name, x in (("clip", clip), ("vf_coef", vf_coef), ("ent_coef", ent_coef)):
            K.number(x, name)
        K.boolean(normalize_advantage, "normalize_advantage")
        K.positive(clip, "clip")
        K.non_negative(vf_coef, "vf_coef")
        K.non_negative(ent_coef, "ent_coef")

    def _ppo_options(self, A, rows, clip_vf, values_old, action_bounds, bounds_coef):
        """What ppo_loss and ppo_grad ask of the options, before anything is launched: the filled pf_ppo_options block, or None where
        both options are off (the call is then the one without options). `rows`: the shapes admitted for values_old."""
        if clip_vf is None:
            if values_old is not None:
                raise ValueError("values_old comes with clip_vf (the range the new values are clipped to around it)")
        else:
            K.number(clip_vf, "clip_vf")
            K.positive(clip_vf, "clip_vf")
            K.tensor(self.device, values_old, "values_old", rows, required="{name} is required with clip_vf: a tensor of shape {shape}")
        K.number(bounds_coef, "bounds_coef")
        K.non_negative(bounds_coef, "bounds_coef")
        lo = hi = None
        if action_bounds is not None:
            try:
                lo, hi = ([float(v) for v in side] for side in action_bounds)
            except (TypeError, ValueError):
                raise ValueError(f"action_bounds must be a pair (low, high) of sequences of {A} numbers, got {action_bounds!r}") from None
            if len(lo) != A or len(hi) != A:
                raise ValueError(f"action_bounds must be a pair (low, high) of sequences of {A} numbers (the action width), got {len(lo)} and {len(hi)}")
            if any(l != l or h != h for l, h in zip(lo, hi)):
                raise ValueError("action_bounds must not hold a NaN (-inf / +inf: open on that side)")
            if any(l > h for l, h in zip(lo, hi)):
                raise ValueError(f"action_bounds: low must be <= high in every column, got {lo} and {hi}")
        elif float(bounds_coef) > 0.0:
            raise ValueError("action_bounds is required with bounds_coef > 0 (the box the means are kept in)")
        bounded = float(bounds_coef) > 0.0
        if clip_vf is None and not bounded:
            return None
        o = L.PfPpoOptions()
        o.clip_vf, o.values_old = (0.0 if clip_vf is None else float(clip_vf)), _ptr(values_old)
        o.bounds_coef = float(bounds_coef)
        for c in range(8):
            o.bounds_lo[c], o.bounds_hi[c] = (lo[c], hi[c]) if bounded and c < A else (float("-inf"), float("inf"))
        return o

    def ppo_loss(self, mean, log_std, value, actions, logp_old, advantages, returns, valid=None, clip: float = 0.2, vf_coef: float = 0.5,
                 ent_coef: float = 0.0, normalize_advantage: bool = True, clip_vf=None, action_bounds=None, bounds_coef: float = 0.0, values_old=None):
        """pf_ppo_loss: the clipped PPO objective of a diagonal-Gaussian policy, its statistics and its gradients with respect to
        mean, value and log_std (include/pyflyt_amd.h has the semantics). mean, actions [..., A] of one shape, A in 1..8; value,
        logp_old, advantages, returns [...] (a trailing axis of 1 is accepted: a critic's output); valid [...] bool / uint8 or None
        (every row valid); all flattened to M = the product of the leading axes, which need not be k n: a gathered minibatch is a
        valid input. Returns (grad_mean [M, A], grad_value [M], grad_log_std [A], stats [16] float64): tensors the engine owns,
        overwritten by the next call with the same M and A (stats and grad_log_std by every call).
        The options (pf_ppo_loss_opt; with the defaults the call is pf_ppo_loss): clip_vf = the range the value loss clips the new
        values to around values_old [...] (the batch's values; required with it); action_bounds = (low, high), two sequences of A
        numbers (an env's action_space.low / .high; -inf / +inf = open), and bounds_coef > 0: the penalty on means outside that box.
        stats[12] is then the fraction of rows outside the value clip range and stats[13] the bounds loss."""
        K.ranked(mean, "mean", "{name} must be a float32 tensor of shape (..., A)")
        A = int(mean.shape[-1])
        if not 1 <= A <= 8:
            raise ValueError(f"mean's last axis (the action width) must be in 1..8, got {A}")
        lead, M = tuple(mean.shape[:-1]), mean.numel() // A
        if M < 1:
            raise ValueError(f"mean must hold at least one row, got shape {tuple(mean.shape)}")
        f32, rows, full = (torch.float32,), (lead, lead + (1,)), (tuple(mean.shape),)  # (this call names its dtypes as torch spells them)
        self._ppo_tensors((("mean", mean, full, f32), ("actions", actions, full, f32), ("log_std", log_std, ((A,),), f32), ("value", value, rows, f32),
                           ("logp_old", logp_old, rows, f32), ("advantages", advantages, rows, f32), ("returns", returns, rows, f32),
                           ("valid", valid, rows, K.FLAGS)))
        self._ppo_coefficients(clip, vf_coef, ent_coef, normalize_advantage)
        options = self._ppo_options(A, rows, clip_vf, values_old, action_bounds, bounds_coef)
        o = self._lazy("_ppo_out", lambda: dict(M=0, A=0, stats=torch.zeros(16, dtype=torch.float64, device=self.device), calls=0))
        if o["M"] != M or o["A"] != A:
            kw = dict(dtype=torch.float32, device=self.device)
            o.update(M=M, A=A, grad_mean=torch.empty(M, A, **kw), grad_value=torch.empty(M, **kw), grad_log_std=torch.empty(A, **kw))
        o["calls"] += 1  # (pyflyt_amd.ppo_loss's backward checks that its gradients are still the ones this call wrote)
        a = L.PfPpoLoss()
        a.clip, a.vf_coef, a.ent_coef, a.normalize_advantage = float(clip), float(vf_coef), float(ent_coef), int(normalize_advantage)
        a.mean, a.log_std, a.actions, a.logp_old = _ptr(mean), _ptr(log_std), _ptr(actions), _ptr(logp_old)
        a.advantages, a.returns, a.value, a.valid = _ptr(advantages), _ptr(returns), _ptr(value), _ptr(valid)
        a.grad_mean, a.grad_value, a.grad_log_std, a.stats = _ptr(o["grad_mean"]), _ptr(o["grad_value"]), _ptr(o["grad_log_std"]), _ptr(o["stats"])
        self._launch(*((self.lib.pf_ppo_loss, C.byref(a)) if options is None else (self.lib.pf_ppo_loss_opt, C.byref(a), C.byref(options))), M, A)
        return o["grad_mean"], o["grad_value"], o["grad_log_std"], o["stats"]

    # ------------------------------------------------------------------ the networks
    def _mlp_block(self, x, layers, activation):
        """The pf_mlp block of `layers` [(weight, bias), ...] for the rows of x [..., in_dim], every tensor checked; returns
        (block, rows, [(out, in), ...])."""
        from .policy import _ACTIVATIONS, MAX_HIDDEN

        if activation not in _ACTIVATIONS:
            raise ValueError(f"activation must be 'tanh' or 'relu', got {activation!r}")
        layers = [tuple(l) for l in layers]
        if len(layers) not in (2, 3):
            raise ValueError(f"layers: 2 or 3 (weight, bias) pairs (1 or 2 hidden layers), got {len(layers)}")
        K.ranked(x, "x", "{name} must be a float32 tensor of shape (..., in_dim)")
        dims = []
        for l, (w, b) in enumerate(layers):
            K.ranked(w, f"layers[{l}].weight", "{name} must be a float32 tensor of shape (out, in)", 2)
            n_out, n_in = int(w.shape[0]), int(w.shape[1])
            want_in = int(x.shape[-1]) if l == 0 else dims[-1][0]
            K.tensor(self.device, w, f"layers[{l}].weight", (n_out, want_in))
            K.tensor(self.device, b, f"layers[{l}].bias", (n_out,), required=K.NO_F32)
            if l + 1 < len(layers) and not 1 <= n_out <= MAX_HIDDEN:
                raise ValueError(f"layers[{l}].weight: hidden width {n_out} is outside 1..{MAX_HIDDEN} (PF_POLICY_MAX_HIDDEN)")
            dims.append((n_out, n_in))
        in_dim, out_dim = dims[0][1], dims[-1][0]
        if not 1 <= in_dim <= 128:
            raise ValueError(f"x's last axis (in_dim) must be in 1..128, got {in_dim}")
        if not 1 <= out_dim <= 8:
            raise ValueError(f"the last layer's width (out_dim) must be in 1..8, got {out_dim}")
        K.tensor(self.device, x, "x", tuple(x.shape))
        rows = x.numel() // in_dim
        if rows < 1:
            raise ValueError(f"x must hold at least one row, got shape {tuple(x.shape)}")
        q = L.PfMlp()
        q.n_layers, q.activation, q.in_dim, q.out_dim = len(layers), _ACTIVATIONS[activation], in_dim, out_dim
        for l in range(2):
            q.width[l] = dims[l][0] if l + 1 < len(layers) else 0
        for l in range(3):
            q.w[l] = layers[l][0].data_ptr() if l < len(layers) else None
            q.b[l] = layers[l][1].data_ptr() if l < len(layers) else None
        return q, rows, dims

    def mlp_forward(self, x, layers, activation="tanh", out=None):
        """pf_mlp_forward: the MLP `layers` [(weight, bias), ...] (torch.nn.Linear's layout; 2 or 3 of them, hidden widths 1..64, the
        last 1..8 wide) on the rows of x [..., in_dim], in_dim 1..128, with policy_act's arithmetic bit for bit. Any engine. Returns
        `out` [rows, out_dim]; without `out`, a tensor the engine owns, overwritten by the next call of the same shape."""
        q, rows, dims = self._mlp_block(x, layers, activation)
        out_dim = dims[-1][0]
        if out is None:
            cache = self._lazy("_mlp_fwd", dict)
            out = cache.get((rows, out_dim))
            if out is None:
                out = cache[(rows, out_dim)] = torch.empty(rows, out_dim, dtype=torch.float32, device=self.device)
        else:
            K.tensor(self.device, out, "out", (rows, out_dim), required=K.NO_F32)
        self._launch(self.lib.pf_mlp_forward, C.byref(q), _ptr(x), rows, _ptr(out))
        return out

    def _grad_tensors(self, dims, gw, gb):
        """[(grad_weight, grad_bias), ...] for layers of the shapes `dims` [(out, in), ...], made here, their addresses written into
        the pointer arrays gw and gb (mlp_backward's own, or those of ppo_grad's argument block)."""
        kw = dict(dtype=torch.float32, device=self.device)
        grads = [(torch.empty(n_out, n_in, **kw), torch.empty(n_out, **kw)) for n_out, n_in in dims]
        for l, (w, b) in enumerate(grads):
            gw[l], gb[l] = w.data_ptr(), b.data_ptr()
        return grads

    def mlp_backward(self, x, grad_out, layers, activation="tanh"):
        """pf_mlp_backward: [(grad_weight, grad_bias), ...] of the MLP `layers` on the rows of x [..., in_dim] under the
        output-gradients grad_out [rows, out_dim] (a [rows] tensor is accepted for out_dim 1). The hidden activations are computed
        again from x; x gets no gradient. The gradients and the workspace are tensors the engine owns, reused by the next call with
        the same rows and layer shapes. Deterministic: the same call gives the same bits on any stream."""
        q, rows, dims = self._mlp_block(x, layers, activation)
        out_dim = dims[-1][0]
        K.tensor(self.device, grad_out, "grad_out", ((rows, out_dim), (rows,)) if out_dim == 1 else (rows, out_dim), required=K.NO_F32)
        cache = self._lazy("_mlp_bwd", dict)
        key = (rows, tuple(dims))
        o = cache.get(key)
        if o is None:
            nbytes = int(self.lib.pf_mlp_backward_workspace_bytes(C.byref(q), rows))
            if nbytes < 1:
                raise L.PyFlytAmdError("pf_mlp_backward_workspace_bytes refused the network's shape")
            gw, gb = (C.c_void_p * 3)(), (C.c_void_p * 3)()
            o = cache[key] = dict(grads=self._grad_tensors(dims, gw, gb), gw=gw, gb=gb, bytes=nbytes,
                                  workspace=torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=self.device))
        self._launch(self.lib.pf_mlp_backward, C.byref(q), _ptr(x), _ptr(grad_out), rows, o["gw"], o["gb"], _ptr(o["workspace"]), o["bytes"])
        return o["grads"]

    def _ppo_grad_inputs(self, x, actor, critic, log_std, actions, logp_old, advantages, returns, valid, clip, vf_coef, ent_coef, normalize_advantage,
                         actor_activation, critic_activation, clip_vf, action_bounds, bounds_coef, values_old, rows):
        """What ppo_grad and ppo_grad_shard check of their inputs, in the order of the refusals. Returns (actor block, critic block, the
        two lists of layer shapes, A, the rows of x, the options block or None, the index list or None, m = the rows the call works on)."""
        index = rows  # (the keyword is the caller's word for it)
        qa, total, dims_a = self._mlp_block(x, actor, actor_activation)
        qc, _, dims_c = self._mlp_block(x, critic, critic_activation)
        A = dims_a[-1][0]
        if dims_c[-1][0] != 1:
            raise ValueError(f"the critic's last layer must be 1 wide, got {dims_c[-1][0]}")
        lead = tuple(x.shape[:-1])
        f32, per_row = (torch.float32,), (lead, lead + (1,), (total,), (total, 1))
        self._ppo_tensors((("log_std", log_std, ((A,),), f32), ("actions", actions, (lead + (A,), (total, A)), f32), ("logp_old", logp_old, per_row, f32),
                           ("advantages", advantages, per_row, f32), ("returns", returns, per_row, f32), ("valid", valid, per_row, K.FLAGS)))
        self._ppo_coefficients(clip, vf_coef, ent_coef, normalize_advantage)
        options = self._ppo_options(A, per_row, clip_vf, values_old, action_bounds, bounds_coef)
        if index is None:
            m = total
        else:  # (the workspace and the cache are those of the m rows the call works on)
            K.ranked(index, "rows", "{name} must be a 1-D int32 tensor of row numbers", 1)
            m = int(index.shape[0])
            if m < 1:
                raise ValueError("rows must name at least one row, got an empty tensor")
            K.tensor(self.device, index, "rows", (m,), torch.int32)
        return qa, qc, dims_a, dims_c, A, total, options, index, m

    def ppo_grad(self, x, actor, critic, log_std, actions, logp_old, advantages, returns, valid=None, clip: float = 0.2, vf_coef: float = 0.5,
                 ent_coef: float = 0.0, normalize_advantage: bool = True, actor_activation="tanh", critic_activation="tanh", clip_vf=None,
                 action_bounds=None, bounds_coef: float = 0.0, values_old=None, rows=None):
        """pf_ppo_grad: what mlp_forward(actor), mlp_forward(critic), ppo_loss, mlp_backward(actor), mlp_backward(critic) give on the
        rows of x [..., in_dim], without the mean, value, grad_mean and grad_value tensors between them (include/pyflyt_amd.h has the
        semantics). actor, critic: [(weight, bias), ...] as for mlp_forward, the critic one wide and on the same in_dim; actions
        [..., A]; logp_old, advantages, returns [...] (a trailing axis of 1 is accepted); valid [...] bool / uint8 or None. Returns
        (actor_grads, critic_grads, grad_log_std [A], stats [16] float64), the first two [(grad_weight, grad_bias), ...]: tensors the
        engine owns, overwritten by the next call with the same rows and layer shapes (stats by every call); so is the workspace.
        clip_vf with values_old [...], action_bounds with bounds_coef: ppo_loss's options (pf_ppo_grad_opt; with the defaults the call
        is pf_ppo_grad).
        rows: None, or a minibatch as a 1-D contiguous int32 tensor [m] of row numbers into the flattened batch (pf_ppo_grad_rows): the
        call is then the one on the m gathered rows, bit for bit, without a gathered copy; the advantages are normalised over those m
        rows; duplicates are allowed; a number outside the batch makes its slot an invalid row and is counted in stats[14]. int64 is
        refused, not converted. The engine's tensors are then those of m rows."""
        qa, qc, dims_a, dims_c, A, total, options, index, m = self._ppo_grad_inputs(
            x, actor, critic, log_std, actions, logp_old, advantages, returns, valid, clip, vf_coef, ent_coef, normalize_advantage, actor_activation,
            critic_activation, clip_vf, action_bounds, bounds_coef, values_old, rows)
        cache = self._lazy("_ppo_grad", lambda: dict(stats=torch.zeros(16, dtype=torch.float64, device=self.device)))
        key = (m, tuple(dims_a), tuple(dims_c))
        o = cache.get(key)
        if o is None:
            nbytes = int(self.lib.pf_ppo_grad_workspace_bytes(C.byref(qa), C.byref(qc), m))
            if nbytes < 1:
                raise L.PyFlytAmdError("pf_ppo_grad_workspace_bytes refused the networks' shapes")
            a = L.PfPpoGradArgs()
            grads = [self._grad_tensors(dims_a, a.actor_grad_w, a.actor_grad_b), self._grad_tensors(dims_c, a.critic_grad_w, a.critic_grad_b)]
            gls = torch.empty(A, dtype=torch.float32, device=self.device)
            a.grad_log_std, a.stats = gls.data_ptr(), cache["stats"].data_ptr()
            o = cache[key] = dict(args=a, grads=grads, grad_log_std=gls, bytes=nbytes, workspace=torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=self.device))
        a = o["args"]
        a.clip, a.vf_coef, a.ent_coef, a.normalize_advantage = float(clip), float(vf_coef), float(ent_coef), int(normalize_advantage)
        a.actor, a.critic = C.addressof(qa), C.addressof(qc)
        a.x, a.log_std, a.actions, a.logp_old = _ptr(x), _ptr(log_std), _ptr(actions), _ptr(logp_old)
        a.advantages, a.returns, a.valid = _ptr(advantages), _ptr(returns), _ptr(valid)
        # the call and what it takes between the argument block and the workspace
        fn, between = ((self.lib.pf_ppo_grad_rows, (None if options is None else C.byref(options), _ptr(index), m, total)) if index is not None
                       else (self.lib.pf_ppo_grad, (m,)) if options is None else (self.lib.pf_ppo_grad_opt, (C.byref(options), m)))
        self._launch(fn, C.byref(a), *between, _ptr(o["workspace"]), o["bytes"])
        return o["grads"][0], o["grads"][1], o["grad_log_std"], cache["stats"]

    # ------------------------------------------------------------------ the sharded gradient (include/pyflyt_amd.h: SHARDED PPO)
    def _flat_grads(self, dims_a, dims_c, flat, gw_a, gb_a, gw_c, gb_c):
        """[(grad_weight, grad_bias), ...] of both networks as views into `flat` [numel] float32, the actor's layers and then the
        critic's, each weight in front of its bias -- the layout ppo_shard_combine's callers share; the views' addresses go into
        the four pointer arrays of a pf_ppo_grad_args block."""
        views, at = [], 0
        for dims, gw, gb in ((dims_a, gw_a, gb_a), (dims_c, gw_c, gb_c)):
            net = []
            for l, (n_out, n_in) in enumerate(dims):
                w = flat[at:at + n_out * n_in].view(n_out, n_in)
                b = flat[at + n_out * n_in:at + n_out * n_in + n_out]
                at += n_out * n_in + n_out
                gw[l], gb[l] = w.data_ptr(), b.data_ptr()
                net.append((w, b))
            views.append(net)
        return views

    @staticmethod
    def grad_numel(dims_a, dims_c):
        """The floats of a flat gradient buffer for networks of the layer shapes [(out, in), ...]."""
        return sum(n_out * n_in + n_out for dims in (dims_a, dims_c) for n_out, n_in in dims)

    def ppo_adv_sums(self, advantages, valid=None, rows=None, out=None):
        """pf_ppo_adv_sums: [4] float64 (valid count, sum A, sum A^2, out-of-range slots) of this shard's rows -- what ppo_grad makes
        c, mu and sigma of, undivided, so that the sums of several shards add up to the joint batch's. advantages [...] float32,
        valid [...] bool / uint8 or None, flattened; rows: None or an int32 index list [m] as for ppo_grad. Returns `out`, or a
        tensor the engine owns, overwritten by the next call."""
        K.ranked(advantages, "advantages", "{name} must be a float32 tensor with at least one axis")
        total = advantages.numel()
        if total < 1:
            raise ValueError(f"advantages must hold at least one row, got shape {tuple(advantages.shape)}")
        K.tensor(self.device, advantages, "advantages", tuple(advantages.shape))
        K.tensor(self.device, valid, "valid", tuple(advantages.shape), K.FLAGS)
        m = total
        if rows is not None:
            K.ranked(rows, "rows", "{name} must be a 1-D int32 tensor of row numbers", 1)
            m = int(rows.shape[0])
            if m < 1:
                raise ValueError("rows must name at least one row, got an empty tensor")
            K.tensor(self.device, rows, "rows", (m,), torch.int32)
        if out is None:
            out = self._lazy("_ppo_shard", dict).setdefault("adv_sums", torch.zeros(4, dtype=torch.float64, device=self.device))
        else:
            K.tensor(self.device, out, "out", (4,), torch.float64)
        self._launch(self.lib.pf_ppo_adv_sums, _ptr(advantages), _ptr(valid), _ptr(rows), m, total, _ptr(out))
        return out

    def _block_list(self, blocks, name, shape, dtype=torch.float64):
        """A list of 1..PF_PPO_MAX_SHARDS tensors of one shape on this device as the (void* x 16) array the sharded calls take."""
        if not isinstance(blocks, (list, tuple)) or not 1 <= len(blocks) <= L.PF_PPO_MAX_SHARDS:
            raise ValueError(f"{name} must be a list of 1..{L.PF_PPO_MAX_SHARDS} tensors (PF_PPO_MAX_SHARDS), got "
                             f"{len(blocks) if isinstance(blocks, (list, tuple)) else type(blocks).__name__}")
        arr = (C.c_void_p * L.PF_PPO_MAX_SHARDS)()
        for g, t in enumerate(blocks):
            K.tensor(self.device, t, f"{name}[{g}]", shape, dtype, required="{name} must be a tensor of shape {shape}")
            arr[g] = t.data_ptr()
        return arr

    def adv_sums_add(self, blocks, out=None):
        """pf_adv_sums_add: the [4] float64 sum of the shards' ppo_adv_sums blocks (copies on this device), added in the list's
        order: the global block every shard's ppo_grad_shard takes. Returns `out`, or a tensor the engine owns."""
        arr = self._block_list(blocks, "blocks", (4,))
        if out is None:
            out = self._lazy("_ppo_shard", dict).setdefault("adv_total", torch.zeros(4, dtype=torch.float64, device=self.device))
        else:
            K.tensor(self.device, out, "out", (4,), torch.float64)
        self._launch(self.lib.pf_adv_sums_add, _ptr(out), arr, len(blocks))
        return out

    def moments_merge(self, dst, blocks):
        """pf_moments_merge: `dst` [1 + 2 D] float64 (count, mean[D], M2[D]) merged in place with the blocks of the same shape, in
        the list's order, by traj_stats' own pairwise update; an empty block changes nothing, an empty dst takes a block's bits.
        Returns dst."""
        K.ranked(dst, "dst", "{name} must be a float64 tensor of shape (1 + 2 D,)", 1)
        D = (int(dst.shape[0]) - 1) // 2
        if dst.shape[0] != 1 + 2 * D or not 1 <= D <= 128:
            raise ValueError(f"dst must hold 1 + 2 D doubles with D in 1..128, got {int(dst.shape[0])}")
        K.tensor(self.device, dst, "dst", (1 + 2 * D,), torch.float64)
        arr = self._block_list(blocks, "blocks", (1 + 2 * D,))
        self._launch(self.lib.pf_moments_merge, _ptr(dst), arr, len(blocks), D)
        return dst

    def ppo_grad_shard(self, x, actor, critic, log_std, actions, logp_old, advantages, returns, adv_sums, valid=None, clip: float = 0.2,
                       vf_coef: float = 0.5, ent_coef: float = 0.0, normalize_advantage: bool = True, actor_activation="tanh", critic_activation="tanh",
                       clip_vf=None, action_bounds=None, bounds_coef: float = 0.0, values_old=None, rows=None):
        """pf_ppo_grad_shard: ppo_grad on this shard's rows with c, mu and sigma of the JOINT batch, taken from adv_sums ([4] float64:
        adv_sums_add's block over all shards, on this device). Returns (actor_grads, critic_grads, flat [numel] float32, block [24]
        float64): the shard's share of the network gradients as views into `flat` (_flat_grads has the layout), and its block of
        raw totals; ppo_shard_combine makes the joint gradients, grad_log_std and stats of the shards' flats and blocks. Tensors the
        engine owns, overwritten by the next call with the same rows and layer shapes; so is the workspace."""
        qa, qc, dims_a, dims_c, A, total, options, index, m = self._ppo_grad_inputs(
            x, actor, critic, log_std, actions, logp_old, advantages, returns, valid, clip, vf_coef, ent_coef, normalize_advantage, actor_activation,
            critic_activation, clip_vf, action_bounds, bounds_coef, values_old, rows)
        K.tensor(self.device, adv_sums, "adv_sums", (4,), torch.float64, required="{name} is required: a tensor of shape {shape}")
        cache = self._lazy("_ppo_shard", dict)
        key = (m, tuple(dims_a), tuple(dims_c))
        o = cache.get(key)
        if o is None:
            nbytes = int(self.lib.pf_ppo_grad_workspace_bytes(C.byref(qa), C.byref(qc), m))
            if nbytes < 1:
                raise L.PyFlytAmdError("pf_ppo_grad_workspace_bytes refused the networks' shapes")
            a = L.PfPpoGradArgs()  # (grad_log_std and stats stay NULL: the combine's outputs)
            flat = torch.empty(self.grad_numel(dims_a, dims_c), dtype=torch.float32, device=self.device)
            grads = self._flat_grads(dims_a, dims_c, flat, a.actor_grad_w, a.actor_grad_b, a.critic_grad_w, a.critic_grad_b)
            o = cache[key] = dict(args=a, grads=grads, flat=flat, block=torch.zeros(L.PF_PPO_SHARD_WORDS, dtype=torch.float64, device=self.device), bytes=nbytes,
                                  workspace=torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=self.device))
        a = o["args"]
        a.clip, a.vf_coef, a.ent_coef, a.normalize_advantage = float(clip), float(vf_coef), float(ent_coef), int(normalize_advantage)
        a.actor, a.critic = C.addressof(qa), C.addressof(qc)
        a.x, a.log_std, a.actions, a.logp_old = _ptr(x), _ptr(log_std), _ptr(actions), _ptr(logp_old)
        a.advantages, a.returns, a.valid = _ptr(advantages), _ptr(returns), _ptr(valid)
        self._launch(self.lib.pf_ppo_grad_shard, C.byref(a), None if options is None else C.byref(options), _ptr(index), m, total, _ptr(adv_sums),
                     _ptr(o["block"]), _ptr(o["workspace"]), o["bytes"])
        return o["grads"][0], o["grads"][1], o["flat"], o["block"]

    def ppo_shard_combine(self, blocks, adv_sums, flats, log_std, vf_coef: float = 0.5, ent_coef: float = 0.0, value_clip: bool = False,
                          bounds_coef: float = 0.0, out=None):
        """pf_ppo_shard_combine: the joint batch's gradients from the shards' ppo_grad_shard outputs, all on this device (copies of
        the other devices'). blocks: the [24] float64 blocks; flats: the [numel] float32 flat gradients, one per shard in the same
        order; adv_sums: the global [4] block; log_std [A]; vf_coef, ent_coef, bounds_coef: the shards'; value_clip: whether they
        ran with clip_vf. Returns (grad [numel] float32 -- `out`, or a tensor the engine owns per numel --, grad_log_std [A],
        stats [16] float64): the sums over the shards in the list's order, and what ppo_grad's finish makes of the summed totals."""
        K.ranked(log_std, "log_std", "{name} must be a float32 tensor of shape (A,)", 1)
        A = int(log_std.shape[0])
        if not 1 <= A <= 8:
            raise ValueError(f"log_std's length (the action width) must be in 1..8, got {A}")
        K.tensor(self.device, log_std, "log_std", (A,))
        K.tensor(self.device, adv_sums, "adv_sums", (4,), torch.float64, required="{name} is required: a tensor of shape {shape}")
        a = L.PfPpoShardCombine()
        a.blocks = self._block_list(blocks, "blocks", (L.PF_PPO_SHARD_WORDS,))
        if not isinstance(flats, (list, tuple)) or len(flats) != len(blocks):
            raise ValueError(f"flats must hold one flat gradient per block ({len(blocks)}), got {len(flats) if isinstance(flats, (list, tuple)) else type(flats).__name__}")
        K.ranked(flats[0], "flats[0]", "{name} must be a 1-D float32 tensor", 1)
        numel = int(flats[0].shape[0])
        if numel < 1:
            raise ValueError("flats[0] must hold at least one element")
        a.grads = self._block_list(flats, "flats", (numel,), torch.float32)
        for name, v in (("vf_coef", vf_coef), ("ent_coef", ent_coef), ("bounds_coef", bounds_coef)):
            K.number(v, name)
            K.non_negative(v, name)
        K.boolean(value_clip, "value_clip")
        cache = self._lazy("_ppo_shard", dict)
        o = cache.get(("combine", numel, A))
        if o is None:
            o = cache[("combine", numel, A)] = dict(grad=torch.empty(numel, dtype=torch.float32, device=self.device),
                                                    grad_log_std=torch.empty(A, dtype=torch.float32, device=self.device),
                                                    stats=torch.zeros(16, dtype=torch.float64, device=self.device))
        if out is None:
            out = o["grad"]
        else:
            K.tensor(self.device, out, "out", (numel,))
        a.n_shards, a.width, a.numel = len(blocks), A, numel
        a.vf_coef, a.ent_coef, a.bounds_coef = float(vf_coef), float(ent_coef), float(bounds_coef)
        a.vclip, a.bnd = int(value_clip), int(float(bounds_coef) > 0.0)
        a.adv_sums, a.log_std = adv_sums.data_ptr(), log_std.data_ptr()
        a.grad_out, a.grad_log_std, a.stats = out.data_ptr(), o["grad_log_std"].data_ptr(), o["stats"].data_ptr()
        self._launch(self.lib.pf_ppo_shard_combine, C.byref(a))
        return out, o["grad_log_std"], o["stats"]

    # ------------------------------------------------------------------ the optimiser
    def adam_step(self, params, grads, exp_avg, exp_avg_sq, state, *, lr=3e-4, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                  max_grad_norm=None, skip_nonfinite: bool = False, gate=None):
        """pf_adam_step: one Adam / AdamW step with global gradient-norm clipping over the tensors `params` (1..32 of them), in
        place, in two launches (include/pyflyt_amd.h has the semantics). grads, exp_avg and exp_avg_sq are lists of tensors shaped
        like the parameters; state is the [8] float64 block (steps, norm, clip coefficient, learning rate, skipped calls), read
        and overwritten. lr is a Python number or a one-element float32 device tensor, read by the kernel at every call.
        max_grad_norm None = no clipping. The hyperparameters reach the kernel as float32. The workspace (one per total size) and
        the filled argument block (one per set of addresses) are the engine's. gate: a one-element int32 / uint32 device tensor
        (kl_control's): the call is then pf_adam_step_gated, and a zero there skips the step on the device (state[5] counts those).
        Returns `state`; nothing synchronises."""
        lists = dict(params=params, grads=grads, exp_avg=exp_avg, exp_avg_sq=exp_avg_sq)
        for name, ts in lists.items():
            if not isinstance(ts, (list, tuple)):
                raise ValueError(f"{name} must be a list of tensors, got {type(ts).__name__}")
        n = len(params)
        if not 1 <= n <= L.PF_ADAM_MAX_TENSORS:
            raise ValueError(f"params: 1..{L.PF_ADAM_MAX_TENSORS} tensors (PF_ADAM_MAX_TENSORS), got {n}")
        for name, ts in lists.items():
            if len(ts) != n:
                raise ValueError(f"{name} must hold one tensor per parameter ({n}), got {len(ts)}")
        lr_dev = lr if torch.is_tensor(lr) else None
        for i, (p, g) in enumerate(zip(params, grads)):  # (the gradients are checked at every call: autograd makes new ones)
            if not torch.is_tensor(p) or not torch.is_tensor(g):  # (one refusal names both: the shape asked of g is p's)
                raise ValueError(f"params[{i}] and grads[{i}] must be tensors, got {type(p).__name__} and {type(g).__name__}")
            K.tensor(self.device, g, f"grads[{i}]", tuple(p.shape))
        key = tuple(t.data_ptr() for ts in lists.values() for t in ts) + (state.data_ptr() if torch.is_tensor(state) else None,
                                                                          None if lr_dev is None else lr_dev.data_ptr())
        cache = self._lazy("_adam", dict)
        o = cache.get(key)
        if o is None:
            for i, p in enumerate(params):
                K.tensor(self.device, p, f"params[{i}]", tuple(p.shape))
                for name in ("exp_avg", "exp_avg_sq"):
                    K.tensor(self.device, lists[name][i], f"{name}[{i}]", tuple(p.shape), required="{name} must be a tensor")
                if p.numel() < 1:
                    raise ValueError(f"params[{i}] must hold at least one element, got shape {tuple(p.shape)}")
            K.tensor(self.device, state, "state", (8,), (torch.float64,), required="{name} must be a float64 tensor of shape {shape}")
            if lr_dev is not None:
                K.tensor(self.device, lr_dev, "lr", tuple(lr_dev.shape) if lr_dev.numel() == 1 else (1,))
            total = sum(p.numel() for p in params)
            nbytes = int(self.lib.pf_adam_workspace_bytes(total))
            if nbytes < 1:
                raise ValueError(f"params: the total number of elements must be below 2^31, got {total}")
            spaces = self._lazy("_adam_ws", dict)
            if total not in spaces:
                spaces[total] = torch.empty(nbytes // 8, dtype=torch.float64, device=self.device)
            a = L.PfAdam()
            a.n_tensors, a.state, a.lr_dev = n, _ptr(state), _ptr(lr_dev)
            for i in range(n):
                a.numel[i] = params[i].numel()
                a.param[i], a.grad[i] = params[i].data_ptr(), grads[i].data_ptr()
                a.exp_avg[i], a.exp_avg_sq[i] = exp_avg[i].data_ptr(), exp_avg_sq[i].data_ptr()
            # (the tensors ride along: an address in the key stays theirs for as long as the entry lives)
            o = cache[key] = dict(args=a, ref=C.byref(a), workspace=_ptr(spaces[total]), bytes=nbytes, keep=(list(params), list(exp_avg), list(exp_avg_sq), state, lr_dev))
            if len(cache) > 64:
                cache.pop(next(iter(cache)))
        K.number(eps, "eps")
        K.number(weight_decay, "weight_decay")
        if lr_dev is None:
            K.number(lr, "lr", " or a one-element float32 device tensor")
        if max_grad_norm is not None:
            K.number(max_grad_norm, "max_grad_norm")
        try:
            b1, b2 = betas
            b1, b2 = float(b1), float(b2)
        except (TypeError, ValueError):
            raise ValueError(f"betas must be a pair of numbers, got {betas!r}") from None
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"betas must lie in [0, 1), got {betas!r}")
        if lr_dev is None:
            K.non_negative(lr, "lr")
        K.positive(eps, "eps")
        K.non_negative(weight_decay, "weight_decay")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError(f"max_grad_norm must be > 0 or None (no clipping), got {max_grad_norm}")
        K.boolean(skip_nonfinite, "skip_nonfinite")
        K.tensor(self.device, gate, "gate", (1,), K.GATE)
        a = o["args"]
        a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = (0.0 if lr_dev is not None else float(lr)), b1, b2, float(eps), float(weight_decay)
        a.max_grad_norm, a.skip_nonfinite = (float("inf") if max_grad_norm is None else float(max_grad_norm)), int(skip_nonfinite)
        with torch.cuda.device(self.device):  # (its own launch code: the raw stream handle, for the host cost of a step)
            if gate is None:
                L.check(self.lib.pf_adam_step(self._ctx, o["ref"], o["workspace"], o["bytes"], C.c_void_p(_raw_stream(self._index))), self._ctx)
            else:
                L.check(self.lib.pf_adam_step_gated(self._ctx, o["ref"], _ptr(gate), o["workspace"], o["bytes"], C.c_void_p(_raw_stream(self._index))), self._ctx)
        return state

    def kl_control(self, stats, gate, state, target_kl, stop_factor: float = 1.5, lr=None, adapt: bool = False, factor: float = 1.5, low: float = 0.5,
                   high: float = 2.0, lr_min: float = 1e-6, lr_max: float = 1e-2):
        """pf_kl_control: the decisions a PPO recipe takes from the measured KL, in one launch of one thread (include/pyflyt_amd.h has
        the semantics). stats: a [16] float64 block of ppo_loss / ppo_grad (slot 5 is read); gate: [1] int32 / uint32, written 1 where
        kl <= stop_factor * target_kl (what adam_step(gate=) reads); state: [4] float64 (kl, lr, gate, closed gates so far). With
        adapt, lr (a one-element float32 device tensor) is divided by `factor` where kl > high * target_kl and multiplied where
        kl < low * target_kl, within [lr_min, lr_max]. Returns `state`; nothing synchronises."""
        need = "{name} is required: a tensor of shape {shape}"
        K.tensor(self.device, stats, "stats", (16,), torch.float64, required=need)
        K.tensor(self.device, gate, "gate", (1,), K.GATE, required=need)
        K.tensor(self.device, state, "state", (4,), torch.float64, required=need)
        K.number(target_kl, "target_kl")
        K.positive(target_kl, "target_kl")
        K.number(stop_factor, "stop_factor")
        if not float(stop_factor) >= 1.0:
            raise ValueError(f"stop_factor must be >= 1 (inf: the gate never closes on a number), got {stop_factor}")
        K.boolean(adapt, "adapt")
        if lr is not None:
            K.tensor(self.device, lr, "lr", tuple(lr.shape) if torch.is_tensor(lr) and lr.numel() == 1 else (1,), required="{name} must be a one-element float32 device tensor")
        if adapt:
            if lr is None:
                raise ValueError("lr (a one-element float32 device tensor) is required with adapt")
            for name, x in (("factor", factor), ("low", low), ("high", high), ("lr_min", lr_min), ("lr_max", lr_max)):
                K.number(x, name)
                K.positive(x, name)
            if not float(factor) > 1.0:
                raise ValueError(f"factor must be > 1, got {factor}")
            if not float(low) < float(high):
                raise ValueError(f"low must be < high, got {low} and {high}")
            if not float(lr_min) <= float(lr_max):
                raise ValueError(f"lr_min must be <= lr_max, got {lr_min} and {lr_max}")
        a = L.PfKlControl()
        a.stats, a.gate, a.state, a.lr_dev = _ptr(stats), _ptr(gate), _ptr(state), _ptr(lr)
        a.target_kl, a.stop_factor, a.adapt = float(target_kl), float(stop_factor), int(adapt)
        a.lr_factor, a.lr_low, a.lr_high, a.lr_min, a.lr_max = float(factor), float(low), float(high), float(lr_min), float(lr_max)
        self._launch(self.lib.pf_kl_control, C.byref(a))
        return state

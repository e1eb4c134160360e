"""BatchEngine: owns the PyTorch-ROCm tensors of one batched simulation and drives the HIP kernels
through the C ABI (include/pyflyt_amd.h). PyTorch is plumbing here -- device memory and streams;
all arithmetic happens in libpyflyt_amd.so.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _checks as K
from . import _lib as L
from .train_ops import TrainOps, _ptr, _raw_stream

_PREPARED_MAX, _PREPARED_BYTES = 256, 256 << 20  # action tensors whose prepared buffer blocks an engine keeps alive, at most (an action ring; a policy's output buffer)


class BatchEngine(TrainOps):
    """N independent drones ("lanes") on one GPU.

    Tensors (all on `device`):
      state      [groups, n, 4] float32  persistent SoA state (float4 groups)
      obs        [n, obs_dim]   float32
      final_obs  [n, obs_dim]   float32  (SAME_STEP auto-reset only)
      reward     [n]            float32
      terminated [n], truncated [n]  bool
    """

    def __init__(self, params: L.PfParams, num_lanes: int, device="cuda:0", lane_offset: int = 0):
        if not torch.cuda.is_available():
            raise L.PyFlytAmdError("pyflyt_amd needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU path")
        self.lib = L.lib()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.PyFlytAmdError(f"device must be a ROCm 'cuda' device, got {device}")
        self.params = params
        self.n = int(num_lanes)
        self.lane_offset = int(lane_offset)
        index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self._ctx = C.c_void_p()
        L.check(self.lib.pf_ctx_create(C.byref(params), self.n, index, self.lane_offset, C.byref(self._ctx)))
        self.groups = self.lib.pf_state_groups(self._ctx)
        self.obs_dim = self.lib.pf_obs_dim(self._ctx)
        # env_step without a mask runs the kernel with its call shape fixed at compile time (include/pyflyt_amd.h: pf_ctx_step_is_fixed)
        self.step_is_fixed = bool(self.lib.pf_ctx_step_is_fixed(self._ctx))
        f32 = dict(dtype=torch.float32, device=self.device)
        self.state = torch.zeros(self.groups, self.n, 4, **f32)
        self.obs = torch.zeros(self.n, self.obs_dim, **f32)
        self.final_obs = torch.zeros(self.n, self.obs_dim, **f32) if params.autoreset == L.AUTORESET_SAME_STEP else None
        # [n, 2] int32 (flags, targets left) of the episode that just ended, before the SAME_STEP re-initialisation
        self.final_info = torch.zeros(self.n, 2, dtype=torch.int32, device=self.device) if params.autoreset == L.AUTORESET_SAME_STEP else None
        self.reward = torch.zeros(self.n, **f32)
        self.terminated = torch.zeros(self.n, dtype=torch.bool, device=self.device)
        self.truncated = torch.zeros(self.n, dtype=torch.bool, device=self.device)
        self.out_state = None
        self.link_pos = None
        self.wind_links = 0
        self.ctrl_ratio = None  # [n] int32: physics ticks per controller update of each drone, or None = uniform
        self.modes = None       # [n] int32: per-drone flight modes (QuadX), or None = the context's mode
        self.start_vel = None   # [n, 3] float32: per-drone spawn velocity for aviary_reset, or None = params
        self.armed = None       # [n] bool: Aviary.set_armed, or None = all armed
        self.out_aux = None
        self.out_contact = None
        self.out_contact_peers = None  # [n] uint8, shared worlds only: bit j = touched drone j of the world (pf_buffers.out_contact_peers)
        self._buf = L.PfBuffers()
        self._index = index
        # env_step's hot path: {id(action tensor): (the tensor, its filled pf_buffers block)} -- see env_step
        self._prepared: dict[int, tuple] = {}
        self._step_fn = self.lib.pf_env_step
        # the tensor that holds every lane's CURRENT observation: self.obs after a reset or a step (and after a world rollout, which
        # copies its last row there), the last trajectory row after a rollout of either other kind -- what rollout_policy's first step
        # acts on (pf_policy.obs0)
        self._cur_obs = self.obs

    def close(self):
        if self._ctx:
            self.lib.pf_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    def _buffers(self, actions=None, xi=None, xi_reset=None, u_targets=None, setpoints=None, start_pose=None, wind=None,
                 wrench=None, actions_out=None):
        # (ctrl_ratio: per-drone control rate, set once by the batched Aviary)
        b = self._buf
        b.state = _ptr(self.state)
        b.actions = _ptr(actions)
        b.obs = _ptr(self.obs)
        b.final_obs = _ptr(self.final_obs)
        b.reward = _ptr(self.reward)
        b.terminated = _ptr(self.terminated)
        b.truncated = _ptr(self.truncated)
        b.xi = _ptr(xi)
        b.xi_reset = _ptr(xi_reset)
        b.u_targets = _ptr(u_targets)
        b.setpoints = _ptr(setpoints)
        b.out_state = _ptr(self.out_state)
        b.out_aux = _ptr(self.out_aux)
        b.out_contact = _ptr(self.out_contact)
        b.start_pose = _ptr(start_pose)
        b.wind = _ptr(wind)
        b.out_link_pos = _ptr(self.link_pos)
        b.ctrl_ratio = _ptr(self.ctrl_ratio)
        b.modes = _ptr(self.modes)
        b.start_vel = _ptr(self.start_vel)
        b.armed = _ptr(self.armed)
        b.final_info = _ptr(self.final_info)
        b.actions_out = _ptr(actions_out)
        b.wrench = _ptr(wrench)
        b.out_contact_peers = _ptr(self.out_contact_peers)
        return b

    @staticmethod
    def _block(src):
        """A private copy of the pf_buffers block `src` (self._buffers(...) fills the ONE shared block, which the next call fills
        again): what outlives the call that made it -- a prepared step, the closed loop's row cursor."""
        b = L.PfBuffers()
        C.memmove(C.byref(b), C.byref(src), C.sizeof(L.PfBuffers))
        return b

    @staticmethod
    def _point_at(b, t):
        """Point the block `b` at the trajectory tensors `t`: a launch that runs all k steps writes their rows itself."""
        b.obs, b.reward, b.terminated, b.truncated = _ptr(t["obs"]), _ptr(t["reward"]), _ptr(t["terminated"]), _ptr(t["truncated"])
        b.final_obs, b.final_info = _ptr(t["final_obs"]), _ptr(t["final_info"])
        return b

    def _sp_dim(self, mode=None):
        """Floats per drone in the setpoint buffer (fixedwing.py:221-224, rocket.py:228): csrc's setpoint_width."""
        mode = self.params.flight_mode if mode is None else mode
        return 7 if self.params.vehicle == L.ROCKET else (6 if (self.params.vehicle == L.FIXEDWING and mode == -1) else 4)

    def _check_per_lane(self):
        K.tensor(self.device, self.ctrl_ratio, "ctrl_ratio", (self.n,), (torch.int32,))
        K.tensor(self.device, self.modes, "modes", (self.n,), (torch.int32,))
        K.tensor(self.device, self.start_vel, "start_vel", (self.n, 3), (torch.float32,))
        K.tensor(self.device, self.armed, "armed", (self.n,), K.FLAGS)

    @property
    def ticks_per_step(self):
        return self.params.env_step_ratio * self.params.ticks_per_control

    @property
    def settle_ticks(self):
        return self.params.settle_steps * self.params.ticks_per_control

    # ------------------------------------------------------------------ env level
    def env_reset(self, mask=None, xi_reset=None, u_targets=None):
        if mask is not None:
            if mask.dtype != torch.bool and mask.dtype != torch.uint8:
                raise ValueError("mask must be a bool/uint8 tensor")
            mask = mask.to(device=self.device).contiguous()
            K.tensor(self.device, mask, "mask", (self.n,), K.FLAGS)
            # (shared worlds: the agents of a world are reset together; the kernels widen a partial selection to the whole world --
            #  no host-side check, which would cost a device synchronisation per masked reset)
        self._check_targets(u_targets)
        K.tensor(self.device, xi_reset, "xi_reset", (self.settle_ticks, self.n))
        b = self._buffers(xi_reset=xi_reset, u_targets=u_targets)
        self._launch(self.lib.pf_env_reset, C.byref(b), _ptr(mask))
        self._cur_obs = self.obs
        ts = self._ts
        if ts is not None:  # (traj_stats' carries: the open episodes of the lanes that were reset are gone)
            for name in ("carry_return", "carry_length", "carry_disc"):
                ts[name].zero_() if mask is None else ts[name].masked_fill_(mask.bool(), 0)
        wd = self._world_done
        if wd is not None:  # (world_sync's latch: the lanes that were reset have an open episode again)
            wd.zero_() if mask is None else wd.masked_fill_(mask.bool(), 0)
        return self.obs

    @property
    def action_dim(self):
        """Width of the env action: 4, 6 for the dogfight task with assisted_flight=False (pf_params.df_action_dim), 7 for
        Rocket-Landing."""
        if self.params.task == L.TASK_ROCKET_LANDING:
            return 7
        return 6 if (self.params.task == L.TASK_DOGFIGHT and self.params.df_action_dim == 6) else 4

    def env_step(self, actions, xi=None, xi_reset=None, u_targets=None):
        """One env step of every lane: pf_env_step on torch's current stream. Results in self.obs / reward / terminated / truncated
        (the same tensors every call). The host cost of a call whose `actions` TENSOR OBJECT this engine has seen before -- a
        policy writing into a fixed buffer, an action ring -- is one dictionary lookup, the raw stream handle and the foreign call:
        the tensor checks and the ~25 pointer conversions are done once per tensor (the prepared block keeps the tensor alive, so
        its id cannot be recycled; its address is compared on every call). Capturable in a HIP graph (no host synchronisation, no allocation)."""
        if xi is None and xi_reset is None and u_targets is None:
            hit = self._prepared.get(id(actions))
            if hit is None or hit[3] != actions.data_ptr():  # (a tensor re-pointed in place -- t.data = ..., set_() -- is prepared again)
                hit = self._prepare(actions)
            rc = self._step_fn(self._ctx, hit[1], _raw_stream(self._index))  # (the library selects the context's device itself)
            if rc:
                L.check(rc, self._ctx)
            self._cur_obs = self.obs
            return self.obs, self.reward, self.terminated, self.truncated
        K.tensor(self.device, actions, "actions", (self.n, self.action_dim))
        K.tensor(self.device, xi, "xi", (self.ticks_per_step, self.n))
        K.tensor(self.device, xi_reset, "xi_reset", (self.settle_ticks, self.n))
        self._check_targets(u_targets)
        b = self._buffers(actions=actions, xi=xi, xi_reset=xi_reset, u_targets=u_targets)
        self._launch(self.lib.pf_env_step, C.byref(b))
        self._cur_obs = self.obs
        return self.obs, self.reward, self.terminated, self.truncated

    def _prepare(self, actions):
        if not torch.is_tensor(actions):
            raise ValueError(f"actions must be a float32 tensor of shape {(self.n, self.action_dim)} on {self.device}, got {type(actions).__name__}")
        K.tensor(self.device, actions, "actions", (self.n, self.action_dim))
        b = self._block(self._buffers(actions=actions))
        if len(self._prepared) >= max(8, min(_PREPARED_MAX, _PREPARED_BYTES // (16 * self.n))):
            self._prepared.clear()
        hit = self._prepared[id(actions)] = (actions, C.byref(b), b, actions.data_ptr())
        return hit

    def prepare_step(self, actions):
        """A prepared env step: validates `actions` ([n, action_dim] float32 on the device) and fills the C buffer block ONCE,
        returns launch(stream_ptr) -- one pf_env_step call on that stream (a ctypes.c_void_p, e.g.
        C.c_void_p(torch.cuda.current_stream().cuda_stream)), results in self.obs / reward / terminated / truncated as for
        env_step. For launch-bound inner loops that re-use their action tensors (a policy writing into a fixed buffer): the
        per-call host cost drops from the tensor checks and ~25 pointer conversions of env_step to the one foreign call.
        PF_NOISE_PHILOX / PF_NOISE_OFF only (the injected-noise protocol passes new tensors every step)."""
        if self.params.noise_mode == L.NOISE_INJECT:
            raise ValueError("prepare_step: PF_NOISE_INJECT passes per-step noise tensors; use env_step")
        K.tensor(self.device, actions, "actions", (self.n, self.action_dim))
        b = self._block(self._buffers(actions=actions))
        fn, ctx, ref, check = self.lib.pf_env_step, self._ctx, C.byref(b), L.check

        def launch(stream_ptr):
            rc = fn(ctx, ref, stream_ptr)
            if rc:
                check(rc, ctx)
            self._cur_obs = self.obs

        launch._keep = (b, actions)  # (the buffer block and the action tensor stay alive with the closure)
        return launch

    def _check_targets(self, u_targets):
        if u_targets is not None:
            # (Rocket-Landing: the reset's six spawn draws)
            rows = 6 if self.params.task == L.TASK_ROCKET_LANDING else (4 if self.params.use_yaw_targets else 3) * self.params.num_targets
            K.tensor(self.device, u_targets, "u_targets", (rows, self.n))

    def sample_actions(self, out, step_index: int):
        K.tensor(self.device, out, "out", (self.n, 7 if self.params.task == L.TASK_ROCKET_LANDING else 4))
        self._launch(self.lib.pf_sample_actions, _ptr(out), int(step_index) & 0xFFFFFFFF)
        return out

    def rollout(self, k_steps: int, step_index0: int = 0, actions=None, store_actions: bool = True):
        """pf_rollout: `k_steps` env steps in one launch, the lanes' state resident in registers between them (every env kernel
        since round 4: the specialised ones, the generic one, the dogfight on either aircraft model). Returns the trajectory
        tensors (obs [k, n, D], reward [k, n], terminated [k, n], truncated [k, n], actions [k, n, 4] or None);
        bit-identical to k x (sample_actions(step_index0 + s) + env_step). `actions`: an open-loop sequence
        [k, n, 4] instead of on-device sampling."""
        k = int(k_steps)
        t = self._traj_tensors(k)
        K.tensor(self.device, actions, "actions", (k, self.n, self.action_dim))
        keep = store_actions and actions is None  # (the kernels sample in registers; the draws are written out only on request)
        b = self._point_at(self._buffers(actions=actions, actions_out=t["actions"] if keep else None), t)
        self._launch(self.lib.pf_rollout, C.byref(b), k, int(step_index0) & 0xFFFFFFFF)
        self._cur_obs = t["obs"][k - 1]
        return t["obs"], t["reward"], t["terminated"], t["truncated"], (t["actions"] if actions is None and store_actions else actions)

    def _traj_tensors(self, k):
        """The trajectory tensors rollout(), rollout_policy() and rollout_policy_steps() share: the cached ones for this k, or new ones."""
        return self._lazy("_traj", lambda: self._new_traj(k, k, mean=False), keep=lambda t: t["k"] == k and t["actions"].shape[-1] == self.action_dim)

    def _new_traj(self, k, obs_rows, mean):
        """Trajectory tensors for k steps. `obs_rows`: k = an observation buffer of the k rows the env writes; k + 1 = collect_rollout's
        `obs_all`, whose row 0 is the observation the first step acts on and whose rows 1 .. k are `obs`. `mean`: with the policy's
        means (the rollouts add theirs on request: _traj_mean)."""
        f32 = dict(dtype=torch.float32, device=self.device)
        obs = torch.empty(obs_rows, self.n, self.obs_dim, **f32)
        t = dict(k=k, obs=obs if obs_rows == k else obs[1:], reward=torch.empty(k, self.n, **f32),
                 terminated=torch.empty(k, self.n, dtype=torch.bool, device=self.device),
                 truncated=torch.empty(k, self.n, dtype=torch.bool, device=self.device),
                 actions=torch.empty(k, self.n, self.action_dim, **f32),
                 final_obs=torch.zeros(k, self.n, self.obs_dim, **f32) if self.final_obs is not None else None,
                 final_info=torch.zeros(k, self.n, 2, dtype=torch.int32, device=self.device) if self.final_info is not None else None)
        if obs_rows != k:
            t["obs_all"] = obs
        if mean:
            self._traj_mean(t)
        return t

    def _traj_mean(self, t):
        """t["mean"] [k, n, action width], made when it is first asked for."""
        mean = t.get("mean")
        if mean is None or mean.shape[-1] != self.action_dim:
            mean = t["mean"] = torch.empty(t["k"], self.n, self.action_dim, dtype=torch.float32, device=self.device)
        return mean

    @staticmethod
    def _check_policy(policy):
        from .policy import MLPPolicy

        if not isinstance(policy, MLPPolicy):
            raise ValueError(f"policy must be a pyflyt_amd.MLPPolicy, got {type(policy).__name__}")

    def _policy_block(self, policy):
        """The pf_policy block of `policy` for this engine (MLPPolicy.fill checks its widths and device)."""
        self._check_policy(policy)
        return policy.fill(L.PfPolicy(), self)

    def rollout_policy(self, policy, k_steps: int, step_index0: int = 0, store_mean: bool = False, outcomes: bool = False, group=None, n_groups: int = 1):
        """pf_rollout_policy: `k_steps` env steps in one launch with every action computed on the device by `policy` (an MLPPolicy)
        from the observation the env has just written -- the closed loop of an on-policy collector. The first step acts on the
        engine's current observation (self.obs after a reset or a step, the last row of the previous rollout). Returns
        (obs [k, n, D], reward [k, n], terminated [k, n], truncated [k, n], actions [k, n, 4]) -- the same tensors as rollout(),
        overwritten by the next call -- and, with store_mean, the policy's means [k, n, 4] as a sixth. `step_index0` keys the
        exploration noise: advance it by k between calls. QuadX-Hover / QuadX-Waypoints on the specialised kernel; everything else
        raises PyFlytAmdError with the library's message -- rollout_policy_steps is the same loop on every env.
        outcomes=True (SAME_STEP only: ValueError otherwise, see _fused_policy) adds one pf_episode_outcomes call on the final_info
        rows behind the launch and appends (outcome [k, n] uint8, outcome_counts [n_groups, 16] int64) to what is returned."""
        K.boolean(outcomes, "outcomes")
        self._fused_policy(True, outcomes)
        return self._rollout_with(self._launch_policy, self._policy_block(policy), int(k_steps), step_index0, store_mean, outcomes, group, n_groups)

    def policy_act(self, policy, step_index: int = 0, obs=None, out=None, mean_out=None):
        """pf_policy_act: `policy` (an MLPPolicy) on `obs` [n, D] (default: the engine's current observation) in one launch, on any
        engine with an env task. Returns the actions [n, action_dim] (`out`, or a new tensor), and with `mean_out` [n, action_dim]
        the pair (actions, mean_out). The same network arithmetic and the same draw as rollout_policy's step `step_index`:
        k x (policy_act(step_index0 + s), env_step) is rollout_policy(k, step_index0) bit for bit where that exists."""
        q = self._policy_block(policy)
        obs = self._cur_obs if obs is None else K.tensor(self.device, obs, "obs", (self.n, self.obs_dim))
        if out is None:
            out = torch.empty(self.n, self.action_dim, dtype=torch.float32, device=self.device)
        K.tensor(self.device, out, "out", (self.n, self.action_dim))
        K.tensor(self.device, mean_out, "mean_out", (self.n, self.action_dim))
        q.obs0 = obs.data_ptr()
        q.mean_out = _ptr(mean_out)
        self._launch(self.lib.pf_policy_act, C.byref(q), _ptr(out), int(step_index) & 0xFFFFFFFF)
        return out if mean_out is None else (out, mean_out)

    # ------------------------------------------------------------------ a pool of policies in one launch
    def _pool_blocks(self, policies, name="policies", most=L.PF_POLICY_POOL_MAX):
        """The pf_policy blocks of a pool (a list of 1..`most` MLPPolicy) as one ctypes array, each filled and checked for this engine."""
        if not isinstance(policies, (list, tuple)) or not 1 <= len(policies) <= most:
            raise ValueError(f"{name}: a pool holds 1..{most} policies, got {len(policies) if isinstance(policies, (list, tuple)) else type(policies).__name__}")
        arr = (L.PfPolicy * len(policies))()
        for p, policy in enumerate(policies):
            self._check_policy(policy)
            policy.fill(arr[p], self)
        return arr

    def _pool_plan_bytes(self, n_policies):
        """pf_policy_pool_plan_bytes for this engine's rows (a pure host function: asked of the library itself, no context)."""
        if isinstance(n_policies, bool) or not isinstance(n_policies, int) or not 1 <= n_policies <= L.PF_POLICY_POOL_MAX:
            raise ValueError(f"n_policies must be an int in 1..{L.PF_POLICY_POOL_MAX}, got {n_policies!r}")
        return int(L.lib().pf_policy_pool_plan_bytes(self.n, n_policies))

    def policy_pool_plan(self, row_policy, n_policies):
        """pf_policy_pool_plan: the plan of a pool launch, a new uint8 tensor (opaque). row_policy [n] int32: the policy of every
        row, 0 .. n_policies - 1; any other value (-1) = no policy, and policy_act_pool leaves that row's outputs alone. Made once
        per assignment of rows to policies; one launch, nothing synchronises."""
        nbytes = self._pool_plan_bytes(n_policies)
        K.tensor(self.device, row_policy, "row_policy", (self.n,), torch.int32, required="{name} is required: an int32 tensor of shape {shape}")
        plan = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self._launch(self.lib.pf_policy_pool_plan, _ptr(row_policy), n_policies, _ptr(plan), nbytes)
        return plan

    def policy_act_pool(self, policies, plan, step_index: int = 0, obs=None, out=None, mean_out=None):
        """pf_policy_act_pool: policy_act for a list of 1..17 MLPPolicy in ONE launch, every row evaluated once by the policy that the
        plan's row_policy names for it (policy_pool_plan). Arguments and return value as policy_act's. Row i of the outputs holds the
        bits of policy_act(policies[row_policy[i]], ...); a row without a policy is not written."""
        arr = self._pool_blocks(policies)
        K.tensor(self.device, plan, "plan", (self._pool_plan_bytes(len(arr)),), torch.uint8,
                 required="{name} is required: policy_pool_plan's uint8 tensor of shape {shape}")
        obs = self._cur_obs if obs is None else K.tensor(self.device, obs, "obs", (self.n, self.obs_dim))
        if out is None:
            out = torch.empty(self.n, self.action_dim, dtype=torch.float32, device=self.device)
        K.tensor(self.device, out, "out", (self.n, self.action_dim))
        K.tensor(self.device, mean_out, "mean_out", (self.n, self.action_dim))
        head = arr[0]  # (a view of the array's first block: its address is the array's)
        head.obs0 = obs.data_ptr()
        head.mean_out = _ptr(mean_out)
        self._launch(self.lib.pf_policy_act_pool, C.byref(head), len(arr), _ptr(plan), plan.numel(), _ptr(out), int(step_index) & 0xFFFFFFFF)
        return out if mean_out is None else (out, mean_out)

    def _closed_loop_pool(self, policies, k_steps, group, n_groups):
        """What rollout_policy_steps asks of a LIST of policies before it touches a tensor; returns ((the pf_policy blocks, row_policy), k):
        row_policy is `group`, or None = every row flies the list's only entry."""
        pool = list(policies)
        if not 1 <= len(pool) <= L.PF_OUTCOME_MAX_GROUPS:
            raise ValueError(f"policy: a pool holds 1..{L.PF_OUTCOME_MAX_GROUPS} policies, got {len(pool)}")
        k = int(k_steps)
        if k < 1:
            raise ValueError(f"k_steps must be >= 1, got {k_steps}")
        self._check_stepwise()
        if n_groups != len(pool) or (group is None and len(pool) > 1):
            raise ValueError(f"policy: a pool of {len(pool)} needs group (which policy flies a lane) and n_groups = {len(pool)}, got n_groups = {n_groups!r}")
        K.tensor(self.device, group, "group", (self.n,), torch.int32)
        return (self._pool_blocks(pool, "policy", L.PF_OUTCOME_MAX_GROUPS), group), k

    def rollout_policy_steps(self, policy, k_steps: int, step_index0: int = 0, store_mean: bool = False, outcomes: bool = False, group=None, n_groups: int = 1):
        """rollout_policy, step by step: k x (pf_policy_act, pf_env_step) into the same trajectory tensors, the same return value.
        Two launches per step instead of one for the whole rollout, on every single-agent env: QuadX, Fixedwing-Waypoints and
        Rocket-Landing, the cascaded flight modes, the generic kernel, the 8-point manifold. Each env step writes straight into its
        trajectory rows (final_obs / final_info rows included under SAME_STEP): nothing is copied. Where rollout_policy runs, the
        results are bit-identical. Needs an auto-reset mode and PF_NOISE_OFF / PF_NOISE_PHILOX (ValueError otherwise) -- so the
        multi-agent tasks (dogfight, multi-agent hover), which exist with auto-reset OFF only, are refused here: their loop is
        rollout_policy_worlds (whole worlds reset on the device), or policy_act and env_step with the culling by hand.
        outcomes=True: every step enqueues pf_episode_outcomes behind pf_env_step (three launches per step), on the step's flag rows
        and on its final_info row under SAME_STEP, on the live state otherwise; (outcome [k, n] uint8, outcome_counts [n_groups, 16]
        int64, zeroed when the call begins) are appended to what is returned. group [n] int32 in 0..n_groups-1: the row a lane counts in.
        `policy` may be a list of 1..16 MLPPolicy with n_groups = its length (and `group`, required for more than one): lane i is
        flown by entry group[i] -- G checkpoints side by side in one batch. One pf_policy_pool_plan before the loop, then per step
        ONE pf_policy_act_pool instead of pf_policy_act; each row has the bits its policy's own pf_policy_act would give it."""
        K.boolean(outcomes, "outcomes")
        if isinstance(policy, (list, tuple)):
            pool, k = self._closed_loop_pool(policy, k_steps, group, n_groups)
            return self._rollout_with(lambda q, t, k, s0, mean, oc=None: self._launch_steps(q, t, k, s0, mean, oc=oc, pool=pool), pool[0][0], k, step_index0,
                                      store_mean, outcomes, group, n_groups)
        q, k, _ = self._closed_loop(policy, k_steps, False)
        return self._rollout_with(self._launch_steps, q, k, step_index0, store_mean, outcomes, group, n_groups)

    def _rollout_with(self, launch, q, k, step_index0, store_mean, outcomes=False, group=None, n_groups=1):
        """Either closed loop into the trajectory tensors the rollouts share, and what both return. (The means are as wide as the
        action: 4 wherever the fused launch exists.)"""
        if outcomes:
            self._outcome_shape(1, True, n_groups, 1, False, False)
        t = self._traj_tensors(k)
        mean = self._traj_mean(t) if store_mean else None
        launch(q, t, k, step_index0, mean, oc=self._outcome_block(t, k, group, n_groups) if outcomes else None)
        out = (t["obs"], t["reward"], t["terminated"], t["truncated"], t["actions"])
        out = out + (mean,) if store_mean else out
        return out + (t["outcome"], t["outcome_counts"]) if outcomes else out

    def _closed_loop(self, policy, k_steps, fused, outcomes=False):
        """What rollout_policy_steps and collect_rollout ask before they touch a tensor; returns (the pf_policy block, k, fused)."""
        self._check_policy(policy)
        k = int(k_steps)
        if k < 1:
            raise ValueError(f"k_steps must be >= 1, got {k_steps}")
        fused = self._fused_policy(fused, outcomes)
        if not fused:
            self._check_stepwise()
        return policy.fill(L.PfPolicy(), self), k, fused

    def _check_stepwise(self):
        """What the stepwise closed loop cannot run, refused before any launch."""
        if self.params.task == L.TASK_NONE:
            raise ValueError("the stepwise policy rollout needs an engine with an env task")
        if self.params.autoreset == L.AUTORESET_OFF:
            raise ValueError("the stepwise policy rollout needs an auto-reset mode (auto-reset disabled: finished lanes would idle for the rest of the rollout)")
        if self.params.noise_mode == L.NOISE_INJECT:
            raise ValueError("the stepwise policy rollout runs under PF_NOISE_OFF / PF_NOISE_PHILOX (PF_NOISE_INJECT passes per-step noise tensors; use policy_act and env_step)")

    def _fused_policy(self, fused, outcomes=False):
        """Which closed loop a `fused` argument selects: None = the fused launch where the library has one for the vehicle and task
        (QuadX-Hover / QuadX-Waypoints, with all its refusals), the stepwise path everywhere else. With `outcomes` the fused launch
        serves under SAME_STEP only, where the final_info rows keep every ended episode's words: elsewhere it holds the flags in
        registers and its next reset overwrites the words behind them inside the launch, so None selects the stepwise loop (the
        same bits, two launches per step more) and True is refused."""
        if fused is not None and not isinstance(fused, bool):
            raise ValueError(f"fused must be None, True or False, got {fused!r}")
        if outcomes and self.params.autoreset != L.AUTORESET_SAME_STEP:
            if fused:
                raise ValueError("fused=True with outcomes=True needs SAME_STEP auto-reset: under NEXT_STEP the fused launch keeps the flags in registers "
                                 "and its resets overwrite the words behind them before anything could read them; fused=None or False runs the "
                                 "stepwise loop, whose results are bit-identical")
            return False
        if fused is None:
            return self.params.vehicle == L.QUADX and self.params.task in (L.TASK_HOVER, L.TASK_WAYPOINTS)
        return fused

    def _launch_steps(self, q, t, k, step_index0, mean, A=None, qo=None, opp_lanes=None, oc=None, pool=None):
        """THE stepwise closed loop: k x (pf_policy_act, pf_env_step) into the trajectory tensors `t`, acting first on the engine's
        current observation -- the act of step s reads the row the env wrote at step s - 1, the env's buffer block (a private copy:
        nothing else sees the row cursor) points at the rows of step s, final_obs / final_info rows included where `t` has them.
        With `A` the lanes are worlds of A (auto-reset OFF): every step adds pf_world_sync on its row and pf_env_reset of the worlds
        that were waiting, whose block points at the observation row of the step; with `qo` and `opp_lanes` the opponent's
        pf_policy_act (the same step index) and one merge come between the act and the step -- `qo` a list of (pf_policy block, the
        [n, 1] bool lanes it flies): one act over all rows and one merge EACH. With `oc` (a pf_outcome_args block: _outcome_block)
        every step ends with pf_episode_outcomes on its flag rows into t["outcome"][s] -- behind pf_env_step, and for worlds behind
        pf_world_sync (it reads valid[s] and the reset mask) and in front of the masked pf_env_reset (it reads the live state); the
        words are the step's final_info row where `t` has one. One device selection and one stream
        handle for all the calls; no allocation inside the loop, nothing synchronises.
        With `pool` (a ctypes array of pf_policy blocks, and row_policy [n] int32 or None = every row flies entry 0) the act of every
        step is ONE pf_policy_act_pool straight into actions[s] (and mean[s]): the plan is made here, once, before the loop, and there
        is no second act, no opponent buffer and no merge (`q` is not used and `qo` is None)."""
        b = self._block(self._buffers())
        lib, ctx, check, qref, bref = self.lib, self._ctx, L.check, C.byref(q), C.byref(b)
        act, step = lib.pf_policy_act, lib.pf_env_step
        n, D, W = self.n, self.obs_dim, self.action_dim
        p_obs, p_act, p_rew = t["obs"].data_ptr(), t["actions"].data_ptr(), t["reward"].data_ptr()
        p_term, p_trunc = t["terminated"].data_ptr(), t["truncated"].data_ptr()
        p_fobs = t["final_obs"].data_ptr() if t["final_obs"] is not None else None
        p_finfo = t["final_info"].data_ptr() if t["final_info"] is not None else None
        p_mean = mean.data_ptr() if mean is not None else None
        if A is not None:
            br, w = self._block(b), L.PfWorldSync()
            sync, reset, brref, wref, p_valid = lib.pf_world_sync, lib.pf_env_reset, C.byref(br), C.byref(w), t["valid"].data_ptr()
            w.done, w.reset_out, w.exclude = self.world_done.data_ptr(), t["reset"].data_ptr(), _ptr(opp_lanes)
            p_mask = C.c_void_p(t["reset"].data_ptr())
        opp = None
        if qo is not None:
            opp = self._lazy("_opp_act", lambda: torch.empty(n, W, dtype=torch.float32, device=self.device), keep=lambda o: o.shape[1] == W)
            p_opp = C.c_void_p(opp.data_ptr())
            for block, _ in qo:
                block.mean_out = None
        if oc is not None:
            outcome, ocref, p_out = lib.pf_episode_outcomes, C.byref(oc), t["outcome"].data_ptr()
            if A is not None:
                oc.world_reset, oc.world_latch = t["reset"].data_ptr(), self.world_outcome.data_ptr()
        if pool is not None:
            arr, row_policy = pool
            if row_policy is None:
                row_policy = torch.zeros(n, dtype=torch.int32, device=self.device)
            plan = self.policy_pool_plan(row_policy, len(arr))
            act_pool, n_pool, p_plan, plan_bytes, head = lib.pf_policy_act_pool, len(arr), C.c_void_p(plan.data_ptr()), plan.numel(), arr[0]
            aref = C.byref(head)  # (entry 0 is a view of the array's first block: its address is the array's)
        cur = self._cur_obs.data_ptr()
        with torch.cuda.device(self.device):
            stream = self._stream()
            for s in range(k):
                step_index = (int(step_index0) + s) & 0xFFFFFFFF
                a = p_act + 4 * n * W * s
                if pool is not None:
                    head.obs0 = cur
                    head.mean_out = p_mean + 4 * n * W * s if p_mean is not None else None
                    rc = act_pool(ctx, aref, n_pool, p_plan, plan_bytes, a, step_index, stream)
                else:
                    q.obs0 = cur
                    q.mean_out = p_mean + 4 * n * W * s if p_mean is not None else None
                    rc = act(ctx, qref, a, step_index, stream)
                if rc:
                    check(rc, ctx)
                if opp is not None:
                    row = t["actions"][s]
                    for block, pick in qo:
                        block.obs0 = cur
                        check(act(ctx, C.byref(block), p_opp, step_index, stream), ctx)
                        torch.where(pick, opp, row, out=row)  # (the merge: one launch on the same stream)
                cur = p_obs + 4 * n * D * s
                b.actions, b.obs, b.reward = a, cur, p_rew + 4 * n * s
                b.terminated, b.truncated = p_term + n * s, p_trunc + n * s
                if p_fobs is not None:
                    b.final_obs, b.final_info = p_fobs + 4 * n * D * s, p_finfo + 8 * n * s
                rc = step(ctx, bref, stream)
                if rc:
                    check(rc, ctx)
                if A is not None:
                    w.terminated, w.truncated, w.reward, w.valid_out = b.terminated, b.truncated, b.reward, p_valid + n * s
                    check(sync(ctx, wref, A, stream), ctx)
                if oc is not None:
                    oc.terminated, oc.truncated, oc.outcome_out = b.terminated, b.truncated, p_out + n * s
                    oc.valid = p_valid + n * s if A is not None else None
                    oc.info = p_finfo + 8 * n * s if p_finfo is not None else None
                    rc = outcome(ctx, ocref, 1, A or 1, stream)
                    if rc:
                        check(rc, ctx)
                if A is not None:
                    br.obs = cur
                    check(reset(ctx, brref, p_mask, stream), ctx)
        if A is None:
            self._cur_obs = t["obs"][k - 1]
        else:
            # the last row becomes self.obs: a masked env_reset (reset_envs) writes the lanes it resets THERE and leaves the others, so
            # the tensor it writes must hold every lane's current observation -- as after an env_step, not k steps old
            self.obs.copy_(t["obs"][k - 1])
            self._cur_obs = self.obs

    def _launch_policy(self, q, t, k, step_index0, mean, oc=None):
        """pf_rollout_policy into the trajectory tensors `t`, acting first on the engine's current observation. With `oc` (SAME_STEP:
        _fused_policy) one pf_episode_outcomes call in the trajectory form behind it, on the final_info rows."""
        q.obs0 = self._cur_obs.data_ptr()
        q.mean_out = mean.data_ptr() if mean is not None else None
        b = self._point_at(self._buffers(actions_out=t["actions"]), t)
        self._launch(self.lib.pf_rollout_policy, C.byref(b), C.byref(q), k, int(step_index0) & 0xFFFFFFFF)
        self._cur_obs = t["obs"][k - 1]
        if oc is not None:
            oc.terminated, oc.truncated, oc.info, oc.outcome_out = _ptr(t["terminated"]), _ptr(t["truncated"]), _ptr(t["final_info"]), _ptr(t["outcome"])
            self._launch(self.lib.pf_episode_outcomes, C.byref(oc), k, 1)

    def _collect_into(self, t, launch):
        """What the collect_* calls share: row 0 of `t`'s obs_all becomes a copy of the engine's current observation (the previous
        call's last row, in this buffer or another, or self.obs) and IS the current observation while launch(t) runs, which leaves
        _cur_obs on the last row it wrote. Refused: the engine's current observation is where it was."""
        cur = self._cur_obs
        t["obs_all"][0].copy_(cur)
        self._cur_obs = t["obs_all"][0]
        try:
            launch(t)
        except L.PyFlytAmdError:
            self._cur_obs = cur
            raise
        return t

    def collect_rollout(self, policy, k_steps: int, step_index0: int = 0, fused=None, outcomes: bool = False, group=None, n_groups: int = 1):
        """rollout_policy for a learner: the same launch (`fused`: None = where the library has it, QuadX-Hover / QuadX-Waypoints, and
        rollout_policy_steps' k x (pf_policy_act, pf_env_step) on every other env; True = the fused launch or its refusal; False =
        the stepwise path -- the act of step s reads row s, the env writes row s + 1) into trajectory tensors of its own whose observations live in ONE buffer
        `obs_all` [k + 1, n, D]. Row 0 is the observation the first step acts on (an n x D copy of the engine's current observation),
        the launch writes rows 1 .. k: obs_all[:-1] are the policy's inputs and obs_all[1:] the next observations, both views -- the
        trajectory is never copied. Returns the dict of tensors (obs_all, obs = obs_all[1:], reward, terminated, truncated, actions,
        mean, final_obs / final_info under SAME_STEP), overwritten by the next call with the same k_steps. outcomes=True adds
        outcome [k, n] uint8 and outcome_counts [n_groups, 16] int64 (this call's episodes) as rollout_policy_steps does -- or, where
        the fused launch serves (SAME_STEP), one pf_episode_outcomes call on the final_info rows behind it; with fused=None outside
        SAME_STEP the stepwise loop runs (_fused_policy)."""
        K.boolean(outcomes, "outcomes")
        q, k, fused = self._closed_loop(policy, k_steps, fused, outcomes)
        if outcomes:
            self._outcome_shape(1, True, n_groups, 1, False, False)
        t = self._lazy("_ctraj", lambda: self._new_traj(k, k + 1, mean=True), keep=lambda t: t["k"] == k)
        oc = self._outcome_block(t, k, group, n_groups) if outcomes else None
        launch = self._launch_policy if fused else self._launch_steps
        return self._collect_into(t, lambda t: launch(q, t, k, step_index0, t["mean"], oc=oc))

    # ------------------------------------------------------------------ multi-agent worlds
    @property
    def world_done(self):
        """[n] uint8, made at first use: world_sync's latch as rollout_policy_worlds keeps it -- 1 = this lane's episode has ended and
        its world has not been reset yet. env_reset() zeroes it, env_reset(mask=...) the masked lanes."""
        return self._lazy("_world_done", lambda: torch.zeros(self.n, dtype=torch.uint8, device=self.device))

    def _check_world(self, agents_per_world):
        A = int(agents_per_world)
        if not 1 <= A <= 64 or self.n % A != 0:
            raise ValueError(f"agents_per_world must be in 1..64 and divide the lane count {self.n}, got {agents_per_world}")
        return A

    def world_sync(self, terminated, truncated, reward, done, agents_per_world, exclude=None, valid_out=None, reset_out=None):
        """pf_world_sync: the world-level auto-reset between two env steps (include/pyflyt_amd.h has the rules). terminated, truncated
        [n] bool / uint8 and reward [n] float32: the row the env step has just written, rewritten in place (zeros where the lane's
        agent had finished before the step); done [n] bool / uint8: the latch, read and rewritten; worlds are `agents_per_world`
        adjacent lanes; exclude [n] bool / uint8 or None: lanes that are never valid. Returns (valid [n], reset mask [n]) --
        `valid_out` / `reset_out`, or bool tensors the engine owns, overwritten by the next call. The mask goes to
        env_reset(mask=...) or pf_env_reset. Any engine; nothing synchronises."""
        A, n = self._check_world(agents_per_world), (self.n,)
        need = "{name} is required: a tensor of shape {shape}"
        K.tensor(self.device, terminated, "terminated", n, K.FLAGS, required=need)
        K.tensor(self.device, truncated, "truncated", n, K.FLAGS, required=need)
        K.tensor(self.device, reward, "reward", n, required=need)
        K.tensor(self.device, done, "done", n, K.FLAGS, required=need)
        K.tensor(self.device, exclude, "exclude", n, K.FLAGS)
        if valid_out is None or reset_out is None:
            o = self._lazy("_world_out", lambda: dict(valid=torch.empty(self.n, dtype=torch.bool, device=self.device),
                                                      reset=torch.empty(self.n, dtype=torch.bool, device=self.device)))
            valid_out, reset_out = (o["valid"] if valid_out is None else valid_out), (o["reset"] if reset_out is None else reset_out)
        K.tensor(self.device, valid_out, "valid_out", n, K.FLAGS, required=need)
        K.tensor(self.device, reset_out, "reset_out", n, K.FLAGS, required=need)
        a = L.PfWorldSync()
        a.terminated, a.truncated, a.reward, a.done = _ptr(terminated), _ptr(truncated), _ptr(reward), _ptr(done)
        a.exclude, a.valid_out, a.reset_out = _ptr(exclude), _ptr(valid_out), _ptr(reset_out)
        self._launch(self.lib.pf_world_sync, C.byref(a), A)
        return valid_out, reset_out

    def _closed_loop_worlds(self, policy, k_steps, agents_per_world, opponent, opponent_lanes, outcomes=False, group=None, n_groups=1, pooled=False):
        """What rollout_policy_worlds and collect_rollout_worlds refuse before they touch a tensor; returns (the policy's pf_policy
        block, the opponents' [(pf_policy block, the [n, 1] bool lanes it flies)] or None, k, A, pool). `opponent`: one MLPPolicy, which flies
        opponent_lanes, or a list of 1..16 (a pool): entry p flies the opponent_lanes whose group is p (a list of one: all of them).
        `pooled`: `pool` is _launch_steps' -- the blocks of [policy] + the opponents, and row_policy = 1 + group on the opponents'
        lanes, 0 on the others -- and the list of opponents is None; otherwise `pool` is None."""
        K.boolean(pooled, "pooled")
        if pooled and opponent is None:
            raise ValueError("pooled=True needs an opponent (one policy or a list): the pool launch flies the learner and its opponents in one act, and without an opponent there is nothing to pool")
        if self.params.task == L.TASK_NONE:
            raise ValueError("the world rollout needs an engine with an env task")
        if self.params.autoreset != L.AUTORESET_OFF:
            raise ValueError("the world rollout runs under auto-reset OFF (the multi-agent envs; pf_world_sync resets whole worlds): "
                             "an env with an auto-reset mode of its own goes through rollout_policy_steps")
        if self.params.noise_mode == L.NOISE_INJECT:
            raise ValueError("the world rollout runs under PF_NOISE_OFF / PF_NOISE_PHILOX (PF_NOISE_INJECT passes per-step noise tensors; use policy_act and env_step)")
        k = int(k_steps)
        if k < 1:
            raise ValueError(f"k_steps must be >= 1, got {k_steps}")
        A = self._check_world(agents_per_world)
        if (opponent is None) != (opponent_lanes is None):
            raise ValueError("opponent and opponent_lanes come together or not at all")
        K.boolean(outcomes, "outcomes")
        pool = list(opponent) if isinstance(opponent, (list, tuple)) else None
        if pool is not None and not 1 <= len(pool) <= L.PF_OUTCOME_MAX_GROUPS:
            raise ValueError(f"opponent: a pool holds 1..{L.PF_OUTCOME_MAX_GROUPS} policies, got {len(pool)}")
        if pool is not None and len(pool) > 1 and (group is None or n_groups != len(pool)):
            raise ValueError(f"opponent: a pool of {len(pool)} needs group (which opponent flies a lane) and n_groups = {len(pool)}, got n_groups = {n_groups!r}")
        if outcomes or group is not None:
            self._outcome_shape(1, True, n_groups, A, True, True)
        q = self._policy_block(policy)
        qo = None
        if opponent is not None:
            blocks = [self._policy_block(p) for p in (pool if pool is not None else [opponent])]
            K.tensor(self.device, opponent_lanes, "opponent_lanes", (self.n,), K.FLAGS, required="{name} must be a bool / uint8 tensor of shape {shape}")
            K.tensor(self.device, group, "group", (self.n,), torch.int32)
            lanes = opponent_lanes.bool()
            if pooled:
                one = torch.ones((), dtype=torch.int32, device=self.device)
                row_policy = torch.where(lanes, one if len(blocks) == 1 else 1 + group, one - 1).contiguous()
                return q, None, k, A, ((L.PfPolicy * (1 + len(blocks)))(q, *blocks), row_policy)
            qo = [(b, (lanes if len(blocks) == 1 else lanes & (group == p)).view(self.n, 1)) for p, b in enumerate(blocks)]
        return q, qo, k, A, None

    def rollout_policy_worlds(self, policy, k_steps: int, agents_per_world: int, step_index0: int = 0, opponent=None, opponent_lanes=None,
                              store_mean: bool = False, outcomes: bool = False, group=None, n_groups: int = 1, pooled: bool = False):
        """The closed loop of the multi-agent envs (dogfight, multi-agent hover: auto-reset OFF), with worlds of `agents_per_world`
        adjacent lanes reset on the device once every agent of them has finished. Step s enqueues pf_policy_act(policy,
        step_index0 + s) on the current observation into actions[s] (and mean[s]); pf_env_step into row s; pf_world_sync on row s,
        which writes valid[s], blanks the rows of the lanes that had finished before and names the worlds that were waiting; and
        pf_env_reset of those worlds with row s as the observation buffer: four launches and pf_world_sync's n-byte device copy; nothing
        synchronises with the host.
        With `opponent` (an MLPPolicy) and `opponent_lanes` ([n] bool / uint8) a second pf_policy_act with the same step index
        and one merge put the opponent's actions on those lanes, which are never valid: six launches and the copy. The last observation row is copied into self.obs, which is the engine's
        current observation afterwards: env_step and a masked env_reset go on from it as after a step. Returns (obs [k, n, D],
        reward, terminated, truncated [k, n], actions [k, n, action width], valid [k, n] bool) and, with store_mean, the policy's
        means as a seventh: tensors the engine owns, overwritten by the next call with the same k. The latch is world_done.
        `opponent` may be a list of 1..16 policies (a pool): entry p flies the opponent_lanes whose `group` ([n] int32) is p, at the
        price of one pf_policy_act over ALL rows and one merge per entry -- P full launches, not P partial ones -- unless pooled=True:
        then the plan of row_policy = where(opponent_lanes, 1 + group, 0) is made once before the loop (pf_policy_pool_plan) and every
        step's act is ONE pf_policy_act_pool over [policy] + the opponents straight into actions[s] (and mean[s]), each row evaluated
        once: four launches per step whatever the pool's size, no second act, no merge. Every returned tensor, the state and the
        counts have the bits of pooled=False, but for `mean` on an opponent's lanes (which are never valid): pooled, it holds that
        opponent's own mean; not pooled, the learner's. pooled=True without an opponent is a ValueError. outcomes=True: every
        step enqueues pf_episode_outcomes between pf_world_sync and the reset (one launch more per step) and (outcome [k, n] uint8,
        outcome_counts [n_groups, 16] int64, zeroed when the call begins, row = group) are appended to what is returned; the world
        latch is world_outcome."""
        q, qo, k, A, pool = self._closed_loop_worlds(policy, k_steps, agents_per_world, opponent, opponent_lanes, outcomes, group, n_groups, pooled)
        t = self._lazy("_wtraj", lambda: self._new_world_traj(k, k), keep=lambda t: t["k"] == k)
        mean = self._traj_mean(t) if store_mean else None
        self._launch_steps(q, t, k, step_index0, mean, A, qo, opponent_lanes, self._outcome_block(t, k, group, n_groups) if outcomes else None, pool)
        out = (t["obs"], t["reward"], t["terminated"], t["truncated"], t["actions"], t["valid"])
        out = out + (mean,) if store_mean else out
        return out + (t["outcome"], t["outcome_counts"]) if outcomes else out

    def collect_rollout_worlds(self, policy, k_steps: int, agents_per_world: int, step_index0: int = 0, opponent=None, opponent_lanes=None,
                               outcomes: bool = False, group=None, n_groups: int = 1, pooled: bool = False):
        """rollout_policy_worlds for a learner, as collect_rollout is rollout_policy_steps': the same loop into trajectory tensors of
        its own whose observations live in ONE buffer obs_all [k + 1, n, D] -- row 0 a copy of the engine's current observation,
        rows 1 .. k written by the env steps (and, on reset steps, by the resets). Returns collect_rollout's dict (obs_all, obs =
        obs_all[1:], reward, terminated, truncated, actions, mean) plus valid [k, n] bool, and with outcomes=True outcome and
        outcome_counts (opponent pools, group, n_groups and pooled as in rollout_policy_worlds)."""
        q, qo, k, A, pool = self._closed_loop_worlds(policy, k_steps, agents_per_world, opponent, opponent_lanes, outcomes, group, n_groups, pooled)
        t = self._lazy("_wctraj", lambda: self._new_world_traj(k, k + 1), keep=lambda t: t["k"] == k)
        oc = self._outcome_block(t, k, group, n_groups) if outcomes else None
        return self._collect_into(t, lambda t: self._launch_steps(q, t, k, step_index0, self._traj_mean(t), A, qo, opponent_lanes, oc, pool))

    def _new_world_traj(self, k, obs_rows):
        t = self._new_traj(k, obs_rows, mean=False)
        t["valid"] = torch.empty(k, self.n, dtype=torch.bool, device=self.device)
        t["reset"] = torch.empty(self.n, dtype=torch.uint8, device=self.device)  # (this step's reset mask: world_sync writes it, the reset reads it)
        return t

    def body_tick(self, wrench, n_ticks: int = 1):
        """pf_body_tick: the free-body tick alone under a held body-frame wrench [n, 6] (force, torque)."""
        self._aviary_outputs()
        K.tensor(self.device, wrench, "wrench", (self.n, 6))
        b = self._buffers(wrench=wrench)
        self._launch(self.lib.pf_body_tick, C.byref(b), int(n_ticks))
        return self.out_state

    # ------------------------------------------------------------------ Aviary level
    def _aviary_outputs(self):
        if self.out_state is None:
            aux = {L.QUADX: 4, L.FIXEDWING: 6, L.ROCKET: 9}[self.params.vehicle]
            self.out_state = torch.zeros(self.n, 12, dtype=torch.float32, device=self.device)
            self.out_aux = torch.zeros(self.n, aux, dtype=torch.float32, device=self.device)
            self.out_contact = torch.zeros(self.n, dtype=torch.bool, device=self.device)
            if self.params.agents_per_world > 1:
                self.out_contact_peers = torch.zeros(self.n, dtype=torch.uint8, device=self.device)
            # world positions of the links a wind field is sampled at (QuadX: body link; Fixedwing: 5 surfaces)
            self.wind_links = int(self.lib.pf_wind_links(self._ctx))
            self.link_pos = torch.zeros(self.n, self.wind_links, 3, dtype=torch.float32, device=self.device)

    def aviary_reset(self, start_pose=None):
        self._aviary_outputs()
        K.tensor(self.device, start_pose, "start_pose", (self.n, 7))
        self._check_per_lane()
        b = self._buffers(start_pose=start_pose)
        self._launch(self.lib.pf_aviary_reset, C.byref(b))
        self.params.flight_mode = 0

    def aviary_set_mode(self, mode: int, setpoints):
        self._aviary_outputs()
        K.tensor(self.device, setpoints, "setpoints", (self.n, self._sp_dim(int(mode))))
        self._check_per_lane()
        b = self._buffers()
        self._launch(self.lib.pf_aviary_set_mode, C.byref(b), int(mode), _ptr(setpoints))
        self.params.flight_mode = int(mode)

    def aviary_step(self, setpoints, n_steps: int = 1, xi=None):
        self._aviary_outputs()
        K.tensor(self.device, setpoints, "setpoints", (self.n, self._sp_dim()))
        K.tensor(self.device, xi, "xi", (int(n_steps) * self.params.ticks_per_control, self.n))
        self._check_per_lane()
        b = self._buffers(setpoints=setpoints, xi=xi)
        self._launch(self.lib.pf_aviary_step, C.byref(b), int(n_steps))
        return self.out_state, self.out_aux

    def aviary_tick(self, setpoints, tick_index: int, wind=None, xi=None):
        """One physics tick of Aviary.step (pf_aviary_tick). `wind`: [n, wind_links, 3] world-frame wind
        as sampled after the previous tick, or None. Fills out_state / out_aux / out_contact (this
        tick's contact verdict) / link_pos (where to sample the field next)."""
        self._aviary_outputs()
        K.tensor(self.device, wind, "wind", (self.n, self.wind_links, 3))
        K.tensor(self.device, xi, "xi", (self.n,))
        K.tensor(self.device, setpoints, "setpoints", (self.n, self._sp_dim()))
        self._check_per_lane()
        b = self._buffers(setpoints=setpoints, xi=xi, wind=wind)
        self._launch(self.lib.pf_aviary_tick, C.byref(b), int(tick_index))
        return self.out_state, self.out_aux

    # ------------------------------------------------------------------ state views
    def ints(self):
        """[n, 4] int32 view: step_count, flags, rng_ctr, n_targets_left."""
        g = 5 if self.params.vehicle == L.FIXEDWING else 6
        return self.state[g].view(torch.int32)

    def flags(self):
        return self.ints()[:, 1]

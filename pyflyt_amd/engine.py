"""BatchEngine: owns the PyTorch-ROCm tensors of one batched simulation and drives the HIP kernels
through the C ABI (include/pyflyt_amd.h). PyTorch is plumbing here -- device memory and streams;
all arithmetic happens in libpyflyt_amd.so.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


try:  # the raw handle of torch's current stream without building a torch.cuda.Stream object (0.2 us against 1.5 us per call)
    _raw_stream = torch._C._cuda_getCurrentRawStream
except AttributeError:  # pragma: no cover
    def _raw_stream(index):
        return torch.cuda.current_stream(index).cuda_stream

_PREPARED_MAX, _PREPARED_BYTES = 256, 256 << 20  # action tensors whose prepared buffer blocks an engine keeps alive, at most (an action ring; a policy's output buffer)


class BatchEngine:
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
        # the tensor that holds every lane's CURRENT observation: self.obs after a reset or a step, the last trajectory row after a
        # rollout of either kind -- what rollout_policy's first step acts on (pf_policy.obs0)
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
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

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

    def _check_f32(self, t, shape, name):
        if t is None:
            return None
        if t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} must be a contiguous float32 tensor of shape {tuple(shape)} on {self.device}, "
                             f"got {t.dtype} {tuple(t.shape)} on {t.device}")
        return t

    def _check(self, t, shape, dtypes, name):
        """Every tensor whose data_ptr() crosses the C ABI is checked here: the kernels index raw pointers, so a wrongly
        sized, typed, placed or strided tensor would read or write out of bounds silently."""
        if t is None:
            return None
        if t.dtype not in dtypes or t.device != self.device or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} must be a contiguous {'/'.join(str(d) for d in dtypes)} tensor of shape {tuple(shape)} on {self.device}, "
                             f"got {t.dtype} {tuple(t.shape)} on {t.device}")
        return t

    def _sp_dim(self, mode=None):
        """Floats per drone in the setpoint buffer (fixedwing.py:221-224, rocket.py:228): csrc's setpoint_width."""
        mode = self.params.flight_mode if mode is None else mode
        return 7 if self.params.vehicle == L.ROCKET else (6 if (self.params.vehicle == L.FIXEDWING and mode == -1) else 4)

    def _check_per_lane(self):
        self._check(self.ctrl_ratio, (self.n,), (torch.int32,), "ctrl_ratio")
        self._check(self.modes, (self.n,), (torch.int32,), "modes")
        self._check(self.start_vel, (self.n, 3), (torch.float32,), "start_vel")
        self._check(self.armed, (self.n,), (torch.bool, torch.uint8), "armed")

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
            self._check(mask, (self.n,), (torch.bool, torch.uint8), "mask")
            # (shared worlds: the agents of a world are reset together; the kernels widen a partial selection to the whole world --
            #  no host-side check, which would cost a device synchronisation per masked reset)
        self._check_targets(u_targets)
        self._check_f32(xi_reset, (self.settle_ticks, self.n), "xi_reset")
        b = self._buffers(xi_reset=xi_reset, u_targets=u_targets)
        with torch.cuda.device(self.device):
            L.check(self.lib.pf_env_reset(self._ctx, C.byref(b), _ptr(mask), self._stream()), self._ctx)
        self._cur_obs = self.obs
        ts = getattr(self, "_ts", None)
        if ts is not None:  # (traj_stats' carries: the open episodes of the lanes that were reset are gone)
            for name in ("carry_return", "carry_length", "carry_disc"):
                ts[name].zero_() if mask is None else ts[name].masked_fill_(mask.bool(), 0)
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
        self._check_f32(actions, (self.n, self.action_dim), "actions")
        self._check_f32(xi, (self.ticks_per_step, self.n), "xi")
        self._check_f32(xi_reset, (self.settle_ticks, self.n), "xi_reset")
        self._check_targets(u_targets)
        b = self._buffers(actions=actions, xi=xi, xi_reset=xi_reset, u_targets=u_targets)
        with torch.cuda.device(self.device):
            L.check(self.lib.pf_env_step(self._ctx, C.byref(b), self._stream()), self._ctx)
        self._cur_obs = self.obs
        return self.obs, self.reward, self.terminated, self.truncated

    def _prepare(self, actions):
        if not torch.is_tensor(actions):
            raise ValueError(f"actions must be a float32 tensor of shape {(self.n, self.action_dim)} on {self.device}, got {type(actions).__name__}")
        self._check_f32(actions, (self.n, self.action_dim), "actions")
        b = L.PfBuffers()
        C.memmove(C.byref(b), C.byref(self._buffers(actions=actions)), C.sizeof(L.PfBuffers))
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
        self._check_f32(actions, (self.n, self.action_dim), "actions")
        b = L.PfBuffers()
        C.memmove(C.byref(b), C.byref(self._buffers(actions=actions)), C.sizeof(L.PfBuffers))
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
            self._check_f32(u_targets, (rows, self.n), "u_targets")

    def sample_actions(self, out, step_index: int):
        self._check_f32(out, (self.n, 7 if self.params.task == L.TASK_ROCKET_LANDING else 4), "out")
        with torch.cuda.device(self.device):
            L.check(self.lib.pf_sample_actions(self._ctx, _ptr(out), int(step_index) & 0xFFFFFFFF, self._stream()), self._ctx)
        return out

    def rollout(self, k_steps: int, step_index0: int = 0, actions=None, store_actions: bool = True):
        """pf_rollout: `k_steps` env steps in one launch, the lanes' state resident in registers between them (every env kernel
        since round 4: the specialised ones, the generic one, the dogfight on either aircraft model). Returns the trajectory
        tensors (obs [k, n, D], reward [k, n], terminated [k, n], truncated [k, n], actions [k, n, 4] or None);
        bit-identical to k x (sample_actions(step_index0 + s) + env_step). `actions`: an open-loop sequence
        [k, n, 4] instead of on-device sampling."""
        k = int(k_steps)
        t = self._traj_tensors(k)
        self._check_f32(actions, (k, self.n, self.action_dim), "actions")
        keep = store_actions and actions is None  # (the kernels sample in registers; the draws are written out only on request)
        b = self._buffers(actions=actions, actions_out=t["actions"] if keep else None)
        b.obs, b.reward, b.terminated, b.truncated = _ptr(t["obs"]), _ptr(t["reward"]), _ptr(t["terminated"]), _ptr(t["truncated"])
        b.final_obs, b.final_info = _ptr(t["final_obs"]), _ptr(t["final_info"])
        with torch.cuda.device(self.device):
            L.check(self.lib.pf_rollout(self._ctx, C.byref(b), k, int(step_index0) & 0xFFFFFFFF, self._stream()), self._ctx)
        self._cur_obs = t["obs"][k - 1]
        return t["obs"], t["reward"], t["terminated"], t["truncated"], (t["actions"] if actions is None and store_actions else actions)

    def _traj_tensors(self, k):
        """The trajectory tensors rollout(), rollout_policy() and rollout_policy_steps() share: the cached ones for this k, or new ones."""
        t = getattr(self, "_traj", None)
        if t is None or t["k"] != k or t["actions"].shape[-1] != self.action_dim:
            f32 = dict(dtype=torch.float32, device=self.device)
            t = dict(k=k, obs=torch.empty(k, self.n, self.obs_dim, **f32), reward=torch.empty(k, self.n, **f32),
                     terminated=torch.empty(k, self.n, dtype=torch.bool, device=self.device),
                     truncated=torch.empty(k, self.n, dtype=torch.bool, device=self.device),
                     actions=torch.empty(k, self.n, self.action_dim, **f32),
                     final_obs=torch.zeros(k, self.n, self.obs_dim, **f32) if self.final_obs is not None else None,
                     final_info=torch.zeros(k, self.n, 2, dtype=torch.int32, device=self.device) if self.final_info is not None else None)
            self._traj = t
        return t

    @staticmethod
    def _check_policy(policy):
        from .policy import MLPPolicy

        if not isinstance(policy, MLPPolicy):
            raise ValueError(f"policy must be a pyflyt_amd.MLPPolicy, got {type(policy).__name__}")

    def _policy_block(self, policy):
        """The pf_policy block of `policy` for this engine (MLPPolicy.fill checks its widths and device)."""
        self._check_policy(policy)
        return policy.fill(L.PfPolicy(), self)

    def rollout_policy(self, policy, k_steps: int, step_index0: int = 0, store_mean: bool = False):
        """pf_rollout_policy: `k_steps` env steps in one launch with every action computed on the device by `policy` (an MLPPolicy)
        from the observation the env has just written -- the closed loop of an on-policy collector. The first step acts on the
        engine's current observation (self.obs after a reset or a step, the last row of the previous rollout). Returns
        (obs [k, n, D], reward [k, n], terminated [k, n], truncated [k, n], actions [k, n, 4]) -- the same tensors as rollout(),
        overwritten by the next call -- and, with store_mean, the policy's means [k, n, 4] as a sixth. `step_index0` keys the
        exploration noise: advance it by k between calls. QuadX-Hover / QuadX-Waypoints on the specialised kernel; everything else
        raises PyFlytAmdError with the library's message -- rollout_policy_steps is the same loop on every env."""
        q = self._policy_block(policy)
        k = int(k_steps)
        t = self._traj_tensors(k)
        mean = None
        if store_mean:
            mean = t.get("mean")
            if mean is None:
                mean = t["mean"] = torch.empty(k, self.n, 4, dtype=torch.float32, device=self.device)
        self._launch_policy(q, t, k, step_index0, mean)
        out = (t["obs"], t["reward"], t["terminated"], t["truncated"], t["actions"])
        return out + (mean,) if store_mean else out

    def policy_act(self, policy, step_index: int = 0, obs=None, out=None, mean_out=None):
        """pf_policy_act: `policy` (an MLPPolicy) on `obs` [n, D] (default: the engine's current observation) in one launch, on any
        engine with an env task. Returns the actions [n, action_dim] (`out`, or a new tensor), and with `mean_out` [n, action_dim]
        the pair (actions, mean_out). The same network arithmetic and the same draw as rollout_policy's step `step_index`:
        k x (policy_act(step_index0 + s), env_step) is rollout_policy(k, step_index0) bit for bit where that exists."""
        q = self._policy_block(policy)
        obs = self._cur_obs if obs is None else self._check_f32(obs, (self.n, self.obs_dim), "obs")
        if out is None:
            out = torch.empty(self.n, self.action_dim, dtype=torch.float32, device=self.device)
        self._check_f32(out, (self.n, self.action_dim), "out")
        self._check_f32(mean_out, (self.n, self.action_dim), "mean_out")
        q.obs0 = obs.data_ptr()
        q.mean_out = _ptr(mean_out)
        with torch.cuda.device(self.device):
            L.check(self.lib.pf_policy_act(self._ctx, C.byref(q), _ptr(out), int(step_index) & 0xFFFFFFFF, self._stream()), self._ctx)
        return out if mean_out is None else (out, mean_out)

    def rollout_policy_steps(self, policy, k_steps: int, step_index0: int = 0, store_mean: bool = False):
        """rollout_policy, step by step: k x (pf_policy_act, pf_env_step) into the same trajectory tensors, the same return value.
        Two launches per step instead of one for the whole rollout, on every single-agent env: QuadX, Fixedwing-Waypoints and
        Rocket-Landing, the cascaded flight modes, the generic kernel, the 8-point manifold. Each env step writes straight into its
        trajectory rows (final_obs / final_info rows included under SAME_STEP): nothing is copied. Where rollout_policy runs, the
        results are bit-identical. Needs an auto-reset mode and PF_NOISE_OFF / PF_NOISE_PHILOX (ValueError otherwise) -- so the
        multi-agent tasks (dogfight, multi-agent hover), which exist with auto-reset OFF only, are refused here: their loop is
        policy_act and env_step, with the culling of finished agents in between."""
        self._check_policy(policy)
        k = int(k_steps)
        if k < 1:
            raise ValueError(f"k_steps must be >= 1, got {k_steps}")
        self._check_stepwise()
        q = policy.fill(L.PfPolicy(), self)
        t = self._traj_tensors(k)
        mean = None
        if store_mean:
            mean = t.get("mean")
            if mean is None or mean.shape[-1] != self.action_dim:
                mean = t["mean"] = torch.empty(k, self.n, self.action_dim, dtype=torch.float32, device=self.device)
        self._launch_policy_steps(q, t, k, step_index0, mean)
        out = (t["obs"], t["reward"], t["terminated"], t["truncated"], t["actions"])
        return out + (mean,) if store_mean else out

    def _check_stepwise(self):
        """What the stepwise closed loop cannot run, refused before any launch."""
        if self.params.task == L.TASK_NONE:
            raise ValueError("the stepwise policy rollout needs an engine with an env task")
        if self.params.autoreset == L.AUTORESET_OFF:
            raise ValueError("the stepwise policy rollout needs an auto-reset mode (auto-reset disabled: finished lanes would idle for the rest of the rollout)")
        if self.params.noise_mode == L.NOISE_INJECT:
            raise ValueError("the stepwise policy rollout runs under PF_NOISE_OFF / PF_NOISE_PHILOX (PF_NOISE_INJECT passes per-step noise tensors; use policy_act and env_step)")

    def _fused_policy(self, fused):
        """Which closed loop a `fused` argument selects: None = the fused launch where the library has one for the vehicle and task
        (QuadX-Hover / QuadX-Waypoints, with all its refusals), the stepwise path everywhere else."""
        if fused is None:
            return self.params.vehicle == L.QUADX and self.params.task in (L.TASK_HOVER, L.TASK_WAYPOINTS)
        if not isinstance(fused, bool):
            raise ValueError(f"fused must be None, True or False, got {fused!r}")
        return fused

    def _launch_policy_steps(self, q, t, k, step_index0, mean):
        """k x (pf_policy_act, pf_env_step) into the trajectory tensors `t`, acting first on the engine's current observation: the
        act of step s reads the row the env wrote at step s - 1, the env's buffer block points at the rows of step s."""
        b = self._buffers()
        act, step, ctx, qref, bref = self.lib.pf_policy_act, self.lib.pf_env_step, self._ctx, C.byref(q), C.byref(b)
        n, D, A = self.n, self.obs_dim, self.action_dim
        p_obs, p_act, p_rew = t["obs"].data_ptr(), t["actions"].data_ptr(), t["reward"].data_ptr()
        p_term, p_trunc = t["terminated"].data_ptr(), t["truncated"].data_ptr()
        p_fobs = t["final_obs"].data_ptr() if t["final_obs"] is not None else None
        p_finfo = t["final_info"].data_ptr() if t["final_info"] is not None else None
        p_mean = mean.data_ptr() if mean is not None else None
        cur = self._cur_obs.data_ptr()
        with torch.cuda.device(self.device):
            stream = self._stream()
            for s in range(k):
                q.obs0 = cur
                q.mean_out = p_mean + 4 * n * A * s if p_mean is not None else None
                a = p_act + 4 * n * A * s
                rc = act(ctx, qref, a, (int(step_index0) + s) & 0xFFFFFFFF, stream)
                if rc:
                    L.check(rc, ctx)
                cur = p_obs + 4 * n * D * s
                b.actions, b.obs, b.reward = a, cur, p_rew + 4 * n * s
                b.terminated, b.truncated = p_term + n * s, p_trunc + n * s
                if p_fobs is not None:
                    b.final_obs, b.final_info = p_fobs + 4 * n * D * s, p_finfo + 8 * n * s
                rc = step(ctx, bref, stream)
                if rc:
                    L.check(rc, ctx)
        self._cur_obs = t["obs"][k - 1]

    def _launch_policy(self, q, t, k, step_index0, mean):
        """pf_rollout_policy into the trajectory tensors `t`, acting first on the engine's current observation."""
        q.obs0 = self._cur_obs.data_ptr()
        q.mean_out = mean.data_ptr() if mean is not None else None
        b = self._buffers(actions_out=t["actions"])
        b.obs, b.reward, b.terminated, b.truncated = _ptr(t["obs"]), _ptr(t["reward"]), _ptr(t["terminated"]), _ptr(t["truncated"])
        b.final_obs, b.final_info = _ptr(t["final_obs"]), _ptr(t["final_info"])
        with torch.cuda.device(self.device):
            L.check(self.lib.pf_rollout_policy(self._ctx, C.byref(b), C.byref(q), k, int(step_index0) & 0xFFFFFFFF, self._stream()), self._ctx)
        self._cur_obs = t["obs"][k - 1]

    def collect_rollout(self, policy, k_steps: int, step_index0: int = 0, fused=None):
        """rollout_policy for a learner: the same launch (`fused`: None = where the library has it, QuadX-Hover / QuadX-Waypoints, and
        rollout_policy_steps' k x (pf_policy_act, pf_env_step) on every other env; True = the fused launch or its refusal; False =
        the stepwise path -- the act of step s reads row s, the env writes row s + 1) into trajectory tensors of its own whose observations live in ONE buffer
        `obs_all` [k + 1, n, D]. Row 0 is the observation the first step acts on (an n x D copy of the engine's current observation),
        the launch writes rows 1 .. k: obs_all[:-1] are the policy's inputs and obs_all[1:] the next observations, both views -- the
        trajectory is never copied. Returns the dict of tensors (obs_all, obs = obs_all[1:], reward, terminated, truncated, actions,
        mean, final_obs / final_info under SAME_STEP), overwritten by the next call with the same k_steps."""
        self._check_policy(policy)
        k = int(k_steps)
        if k < 1:
            raise ValueError(f"k_steps must be >= 1, got {k_steps}")
        fused = self._fused_policy(fused)
        if not fused:
            self._check_stepwise()
        q = policy.fill(L.PfPolicy(), self)
        t = getattr(self, "_ctraj", None)
        if t is None or t["k"] != k:
            f32 = dict(dtype=torch.float32, device=self.device)
            obs_all = torch.empty(k + 1, self.n, self.obs_dim, **f32)
            t = dict(k=k, obs_all=obs_all, obs=obs_all[1:], reward=torch.empty(k, self.n, **f32),
                     terminated=torch.empty(k, self.n, dtype=torch.bool, device=self.device),
                     truncated=torch.empty(k, self.n, dtype=torch.bool, device=self.device),
                     actions=torch.empty(k, self.n, self.action_dim, **f32), mean=torch.empty(k, self.n, self.action_dim, **f32),
                     final_obs=torch.zeros(k, self.n, self.obs_dim, **f32) if self.final_obs is not None else None,
                     final_info=torch.zeros(k, self.n, 2, dtype=torch.int32, device=self.device) if self.final_info is not None else None)
            self._ctraj = t
        cur = self._cur_obs
        t["obs_all"][0].copy_(cur)  # (the previous call's last row, in this buffer or another, or self.obs)
        self._cur_obs = t["obs_all"][0]
        try:
            (self._launch_policy if fused else self._launch_policy_steps)(q, t, k, step_index0, t["mean"])
        except L.PyFlytAmdError:  # (refused: the engine's current observation is where it was)
            self._cur_obs = cur
            raise
        return t

    def gae(self, reward, terminated, truncated, values, gamma: float = 0.99, lam: float = 0.95, final_values=None, episode_start=None,
            actions=None, mean=None, log_std=None):
        """pf_gae: which steps of a trajectory are real transitions, their advantages and returns by generalised advantage
        estimation, and the log-probabilities of the actions (include/pyflyt_amd.h has the semantics). reward / terminated /
        truncated [k, n] as a rollout wrote them; values [k + 1, n]: row s the value of the observation the policy saw at step s,
        row k that of the last observation; final_values [k, n]: the value of final_obs, SAME_STEP only (and required there);
        episode_start [n]: NEXT_STEP only, lanes that were waiting for their reset when the rollout began; actions, mean [k, n, A]
        and log_std [A] together, or none of them (then logp is None). Returns (advantages [k, n], returns [k, n], logp [k, n] or
        None, valid [k, n] bool): tensors the engine owns, overwritten by the next call with the same k."""
        if not torch.is_tensor(reward) or reward.dim() != 2:
            raise ValueError(f"reward must be a float32 tensor of shape (k, {self.n}), got {type(reward).__name__ if not torch.is_tensor(reward) else tuple(reward.shape)}")
        k, A = int(reward.shape[0]), self.action_dim
        if k < 1:
            raise ValueError("reward must hold at least one step")
        flags = (torch.bool, torch.uint8)
        self._check_f32(reward, (k, self.n), "reward")
        for name, x in (("terminated", terminated), ("truncated", truncated)):
            if x is None:
                raise ValueError(f"{name} is required")
            self._check(x, (k, self.n), flags, name)
        if values is None:
            raise ValueError("values is required")
        self._check_f32(values, (k + 1, self.n), "values")
        for name, x in (("gamma", gamma), ("lam", lam)):
            if not 0.0 <= float(x) <= 1.0:  # (False for a NaN as well)
                raise ValueError(f"{name} must be finite and in [0, 1], got {x}")
        same, nxt = self.params.autoreset == L.AUTORESET_SAME_STEP, self.params.autoreset == L.AUTORESET_NEXT_STEP
        if same and final_values is None:
            raise ValueError("final_values is required under SAME_STEP auto-reset (the value of the terminal observation in final_obs)")
        if not same and final_values is not None:
            raise ValueError("final_values must be None outside SAME_STEP auto-reset (there is no final_obs)")
        if not nxt and episode_start is not None:
            raise ValueError("episode_start must be None outside NEXT_STEP auto-reset (no other mode has reset steps)")
        self._check_f32(final_values, (k, self.n), "final_values")
        self._check(episode_start, (self.n,), flags, "episode_start")
        given = [x is not None for x in (actions, mean, log_std)]
        if any(given) and not all(given):
            raise ValueError("actions, mean and log_std come together or not at all")
        self._check_f32(actions, (k, self.n, A), "actions")
        self._check_f32(mean, (k, self.n, A), "mean")
        self._check_f32(log_std, (A,), "log_std")
        o = getattr(self, "_gae_out", None)
        if o is None or o["k"] != k:
            f32 = dict(dtype=torch.float32, device=self.device)
            o = self._gae_out = dict(k=k, advantages=torch.empty(k, self.n, **f32), returns=torch.empty(k, self.n, **f32),
                                     logp=torch.empty(k, self.n, **f32), valid=torch.empty(k, self.n, dtype=torch.bool, device=self.device))
        a = L.PfGae()
        a.gamma = float(gamma)
        setattr(a, "lambda", float(lam))
        a.reward, a.terminated, a.truncated, a.values = _ptr(reward), _ptr(terminated), _ptr(truncated), _ptr(values)
        a.final_values, a.episode_start = _ptr(final_values), _ptr(episode_start)
        a.actions, a.mean, a.log_std = _ptr(actions), _ptr(mean), _ptr(log_std)
        a.advantages, a.returns, a.valid_out = _ptr(o["advantages"]), _ptr(o["returns"]), _ptr(o["valid"])
        a.logp_out = _ptr(o["logp"]) if all(given) else None
        with torch.cuda.device(self.device):
            L.check(self.lib.pf_gae(self._ctx, C.byref(a), k, self._stream()), self._ctx)
        return o["advantages"], o["returns"], (o["logp"] if all(given) else None), o["valid"]

    def _traj_state(self):
        """What traj_stats keeps between calls, made at its first use: the per-lane carries, summary and the two running moment blocks."""
        ts = getattr(self, "_ts", None)
        if ts is None:
            f32, f64 = dict(dtype=torch.float32, device=self.device), dict(dtype=torch.float64, device=self.device)
            ts = self._ts = dict(carry_return=torch.zeros(self.n, **f32), carry_length=torch.zeros(self.n, dtype=torch.int32, device=self.device),
                                 carry_disc=torch.zeros(self.n, **f32), summary=torch.zeros(8, **f64),
                                 obs_moments=torch.zeros(1 + 2 * self.obs_dim, **f64), ret_moments=torch.zeros(3, **f64), k=0)
        return ts

    @property
    def obs_moments(self):
        """[1 + 2 D] float64 (count, mean[D], M2[D]): the running moments of the observation columns (traj_stats with obs=)."""
        return self._traj_state()["obs_moments"]

    @property
    def ret_moments(self):
        """[3] float64 (count, mean, M2): the running moments of the discounted return G (traj_stats)."""
        return self._traj_state()["ret_moments"]

    def reset_moments(self):
        """Zero the running moments of traj_stats (the empty state). The carries of the open episodes stay."""
        ts = self._traj_state()
        ts["obs_moments"].zero_()
        ts["ret_moments"].zero_()

    def traj_stats(self, reward, terminated, truncated, gamma: float = 0.99, episode_start=None, obs=None, store_steps: bool = True):
        """pf_traj_stats: the return and length of every episode that finished inside a trajectory, and the running moments of a
        reward and an observation normaliser (include/pyflyt_amd.h has the semantics). reward / terminated / truncated [k, n] as a
        rollout wrote them; episode_start [n]: NEXT_STEP only, as for gae(); obs [k, n, D]: the observations the policy saw (collect's
        obs), or None for no observation moments; store_steps=False skips the two per-step outputs. The engine owns the per-lane
        carries (a trajectory may be split over calls; env_reset zeroes the lanes it resets), summary and the running moments
        (self.obs_moments, self.ret_moments; reset_moments() empties them). The carries describe the lanes' open episodes only if
        EVERY env step since the last reset goes through traj_stats, in order: steps taken by env_step, rollout or a collect without
        stats in between are not seen, and the next finished episode's return and length would miss them -- reset the lanes (or
        zero the carries) before mixing the two. Returns (episode_return [k, n], episode_length [k, n]
        int32 -- both None without store_steps --, summary [8] float64): overwritten by the next call with the same k."""
        if not torch.is_tensor(reward) or reward.dim() != 2:
            raise ValueError(f"reward must be a float32 tensor of shape (k, {self.n}), got {type(reward).__name__ if not torch.is_tensor(reward) else tuple(reward.shape)}")
        k = int(reward.shape[0])
        if k < 1:
            raise ValueError("reward must hold at least one step")
        flags = (torch.bool, torch.uint8)
        self._check_f32(reward, (k, self.n), "reward")
        for name, x in (("terminated", terminated), ("truncated", truncated)):
            if x is None:
                raise ValueError(f"{name} is required")
            self._check(x, (k, self.n), flags, name)
        if not 0.0 <= float(gamma) <= 1.0:  # (False for a NaN as well)
            raise ValueError(f"gamma must be finite and in [0, 1], got {gamma}")
        if self.params.autoreset != L.AUTORESET_NEXT_STEP and episode_start is not None:
            raise ValueError("episode_start must be None outside NEXT_STEP auto-reset (no other mode has reset steps)")
        self._check(episode_start, (self.n,), flags, "episode_start")
        if obs is not None and not torch.is_tensor(obs):
            raise ValueError(f"obs must be a float32 tensor of shape (k, {self.n}, D), got {type(obs).__name__}")
        if obs is not None:
            self._check_f32(obs, (k, self.n, self.obs_dim), "obs")
        ts = self._traj_state()
        if store_steps and ts["k"] != k:
            ts.update(k=k, episode_return=torch.empty(k, self.n, dtype=torch.float32, device=self.device),
                      episode_length=torch.empty(k, self.n, dtype=torch.int32, device=self.device))
        a = L.PfTrajStats()
        a.gamma = float(gamma)
        a.reward, a.terminated, a.truncated, a.episode_start = _ptr(reward), _ptr(terminated), _ptr(truncated), _ptr(episode_start)
        a.obs, a.obs_moments = _ptr(obs), (_ptr(ts["obs_moments"]) if obs is not None else None)
        a.carry_return, a.carry_length, a.carry_disc = _ptr(ts["carry_return"]), _ptr(ts["carry_length"]), _ptr(ts["carry_disc"])
        a.ep_return_out = _ptr(ts["episode_return"]) if store_steps else None
        a.ep_length_out = _ptr(ts["episode_length"]) if store_steps else None
        a.summary, a.ret_moments = _ptr(ts["summary"]), _ptr(ts["ret_moments"])
        with torch.cuda.device(self.device):
            L.check(self.lib.pf_traj_stats(self._ctx, C.byref(a), k, self._stream()), self._ctx)
        return (ts["episode_return"] if store_steps else None), (ts["episode_length"] if store_steps else None), ts["summary"]

    def ppo_loss(self, mean, log_std, value, actions, logp_old, advantages, returns, valid=None, clip: float = 0.2, vf_coef: float = 0.5,
                 ent_coef: float = 0.0, normalize_advantage: bool = True):
        """pf_ppo_loss: the clipped PPO objective of a diagonal-Gaussian policy, its statistics and its gradients with respect to
        mean, value and log_std (include/pyflyt_amd.h has the semantics). mean, actions [..., A] of one shape, A in 1..8; value,
        logp_old, advantages, returns [...] (a trailing axis of 1 is accepted: a critic's output); valid [...] bool / uint8 or None
        (every row valid); all flattened to M = the product of the leading axes, which need not be k n: a gathered minibatch is a
        valid input. Returns (grad_mean [M, A], grad_value [M], grad_log_std [A], stats [16] float64): tensors the engine owns,
        overwritten by the next call with the same M and A (stats and grad_log_std by every call)."""
        if not torch.is_tensor(mean) or mean.dim() < 1:
            raise ValueError(f"mean must be a float32 tensor of shape (..., A), got {type(mean).__name__ if not torch.is_tensor(mean) else tuple(mean.shape)}")
        A = int(mean.shape[-1])
        if not 1 <= A <= 8:
            raise ValueError(f"mean's last axis (the action width) must be in 1..8, got {A}")
        lead = tuple(mean.shape[:-1])
        M = 1
        for d in lead:
            M *= int(d)
        if M < 1:
            raise ValueError(f"mean must hold at least one row, got shape {tuple(mean.shape)}")

        def flat(t, shapes, dtypes, name):
            if not torch.is_tensor(t):
                raise ValueError(f"{name} is required: a tensor of shape {shapes[0]}, got {type(t).__name__}")
            if t.dtype not in dtypes or t.device != self.device or not t.is_contiguous() or tuple(t.shape) not in shapes:
                raise ValueError(f"{name} must be a contiguous {'/'.join(str(d) for d in dtypes)} tensor of shape {shapes[0]} on {self.device}, "
                                 f"got {t.dtype} {tuple(t.shape)} on {t.device}")
            return t

        f32, rows = (torch.float32,), (lead, lead + (1,))
        flat(mean, (tuple(mean.shape),), f32, "mean")
        flat(actions, (tuple(mean.shape),), f32, "actions")
        flat(log_std, ((A,),), f32, "log_std")
        for name, x in (("value", value), ("logp_old", logp_old), ("advantages", advantages), ("returns", returns)):
            flat(x, rows, f32, name)
        if valid is not None:
            flat(valid, rows, (torch.bool, torch.uint8), "valid")
        for name, x in (("clip", clip), ("vf_coef", vf_coef), ("ent_coef", ent_coef)):
            if isinstance(x, bool) or not isinstance(x, (int, float)):
                raise ValueError(f"{name} must be a Python number, got {type(x).__name__}")
        if not isinstance(normalize_advantage, bool):
            raise ValueError(f"normalize_advantage must be a bool, got {type(normalize_advantage).__name__}")
        if not 0.0 < float(clip) < float("inf"):  # (False for a NaN as well)
            raise ValueError(f"clip must be finite and > 0, got {clip}")
        for name, x in (("vf_coef", vf_coef), ("ent_coef", ent_coef)):
            if not 0.0 <= float(x) < float("inf"):
                raise ValueError(f"{name} must be finite and >= 0, got {x}")
        o = getattr(self, "_ppo_out", None)
        if o is None:
            o = self._ppo_out = dict(M=0, A=0, stats=torch.zeros(16, dtype=torch.float64, device=self.device), calls=0)
        if o["M"] != M or o["A"] != A:
            kw = dict(dtype=torch.float32, device=self.device)
            o.update(M=M, A=A, grad_mean=torch.empty(M, A, **kw), grad_value=torch.empty(M, **kw), grad_log_std=torch.empty(A, **kw))
        o["calls"] += 1  # (pyflyt_amd.ppo_loss's backward checks that its gradients are still the ones this call wrote)
        a = L.PfPpoLoss()
        a.clip, a.vf_coef, a.ent_coef, a.normalize_advantage = float(clip), float(vf_coef), float(ent_coef), int(normalize_advantage)
        a.mean, a.log_std, a.actions, a.logp_old = _ptr(mean), _ptr(log_std), _ptr(actions), _ptr(logp_old)
        a.advantages, a.returns, a.value, a.valid = _ptr(advantages), _ptr(returns), _ptr(value), _ptr(valid)
        a.grad_mean, a.grad_value, a.grad_log_std, a.stats = _ptr(o["grad_mean"]), _ptr(o["grad_value"]), _ptr(o["grad_log_std"]), _ptr(o["stats"])
        with torch.cuda.device(self.device):
            L.check(self.lib.pf_ppo_loss(self._ctx, C.byref(a), M, A, self._stream()), self._ctx)
        return o["grad_mean"], o["grad_value"], o["grad_log_std"], o["stats"]

    def _mlp_block(self, x, layers, activation):
        """The pf_mlp block of `layers` [(weight, bias), ...] for the rows of x [..., in_dim], every tensor checked; returns
        (block, rows, [(out, in), ...])."""
        from .policy import _ACTIVATIONS, MAX_HIDDEN

        if activation not in _ACTIVATIONS:
            raise ValueError(f"activation must be 'tanh' or 'relu', got {activation!r}")
        layers = [tuple(l) for l in layers]
        if len(layers) not in (2, 3):
            raise ValueError(f"layers: 2 or 3 (weight, bias) pairs (1 or 2 hidden layers), got {len(layers)}")
        if not torch.is_tensor(x) or x.dim() < 1:
            raise ValueError(f"x must be a float32 tensor of shape (..., in_dim), got {type(x).__name__ if not torch.is_tensor(x) else tuple(x.shape)}")
        dims = []
        for l, (w, b) in enumerate(layers):
            if not torch.is_tensor(w) or w.dim() != 2:
                raise ValueError(f"layers[{l}].weight must be a float32 tensor of shape (out, in), got {type(w).__name__ if not torch.is_tensor(w) else tuple(w.shape)}")
            n_out, n_in = int(w.shape[0]), int(w.shape[1])
            want_in = int(x.shape[-1]) if l == 0 else dims[-1][0]
            self._check_f32(w, (n_out, want_in), f"layers[{l}].weight")
            if not torch.is_tensor(b):
                raise ValueError(f"layers[{l}].bias must be a float32 tensor of shape ({n_out},), got {type(b).__name__}")
            self._check_f32(b, (n_out,), f"layers[{l}].bias")
            if l + 1 < len(layers) and not 1 <= n_out <= MAX_HIDDEN:
                raise ValueError(f"layers[{l}].weight: hidden width {n_out} is outside 1..{MAX_HIDDEN} (PF_POLICY_MAX_HIDDEN)")
            dims.append((n_out, n_in))
        in_dim, out_dim = dims[0][1], dims[-1][0]
        if not 1 <= in_dim <= 128:
            raise ValueError(f"x's last axis (in_dim) must be in 1..128, got {in_dim}")
        if not 1 <= out_dim <= 8:
            raise ValueError(f"the last layer's width (out_dim) must be in 1..8, got {out_dim}")
        self._check_f32(x, tuple(x.shape), "x")
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
            cache = self.__dict__.setdefault("_mlp_fwd", {})
            out = cache.get((rows, out_dim))
            if out is None:
                out = cache[(rows, out_dim)] = torch.empty(rows, out_dim, dtype=torch.float32, device=self.device)
        else:
            if not torch.is_tensor(out):
                raise ValueError(f"out must be a float32 tensor of shape {(rows, out_dim)}, got {type(out).__name__}")
            self._check_f32(out, (rows, out_dim), "out")
        with torch.cuda.device(self.device):
            L.check(self.lib.pf_mlp_forward(self._ctx, C.byref(q), _ptr(x), rows, _ptr(out), self._stream()), self._ctx)
        return out

    def mlp_backward(self, x, grad_out, layers, activation="tanh"):
        """pf_mlp_backward: [(grad_weight, grad_bias), ...] of the MLP `layers` on the rows of x [..., in_dim] under the
        output-gradients grad_out [rows, out_dim] (a [rows] tensor is accepted for out_dim 1). The hidden activations are computed
        again from x; x gets no gradient. The gradients and the workspace are tensors the engine owns, reused by the next call with
        the same rows and layer shapes. Deterministic: the same call gives the same bits on any stream."""
        q, rows, dims = self._mlp_block(x, layers, activation)
        out_dim = dims[-1][0]
        if not torch.is_tensor(grad_out):
            raise ValueError(f"grad_out must be a float32 tensor of shape {(rows, out_dim)}, got {type(grad_out).__name__}")
        self._check_f32(grad_out, tuple(grad_out.shape) if out_dim == 1 and tuple(grad_out.shape) == (rows,) else (rows, out_dim), "grad_out")
        cache = self.__dict__.setdefault("_mlp_bwd", {})
        key = (rows, tuple(dims))
        o = cache.get(key)
        if o is None:
            kw = dict(dtype=torch.float32, device=self.device)
            nbytes = int(self.lib.pf_mlp_backward_workspace_bytes(C.byref(q), rows))
            if nbytes < 1:
                raise L.PyFlytAmdError("pf_mlp_backward_workspace_bytes refused the network's shape")
            grads = [(torch.empty(n_out, n_in, **kw), torch.empty(n_out, **kw)) for n_out, n_in in dims]
            gw, gb = (C.c_void_p * 3)(), (C.c_void_p * 3)()
            for l, (w, b) in enumerate(grads):
                gw[l], gb[l] = w.data_ptr(), b.data_ptr()
            o = cache[key] = dict(grads=grads, gw=gw, gb=gb, bytes=nbytes, workspace=torch.empty((nbytes + 3) // 4, **kw))
        with torch.cuda.device(self.device):
            L.check(self.lib.pf_mlp_backward(self._ctx, C.byref(q), _ptr(x), _ptr(grad_out), rows, o["gw"], o["gb"], _ptr(o["workspace"]), o["bytes"],
                                             self._stream()), self._ctx)
        return o["grads"]

    def adam_step(self, params, grads, exp_avg, exp_avg_sq, state, *, lr=3e-4, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                  max_grad_norm=None, skip_nonfinite: bool = False):
        """pf_adam_step: one Adam / AdamW step with global gradient-norm clipping over the tensors `params` (1..32 of them), in
        place, in two launches (include/pyflyt_amd.h has the semantics). grads, exp_avg and exp_avg_sq are lists of tensors shaped
        like the parameters; state is the [8] float64 block (steps, norm, clip coefficient, learning rate, skipped calls), read
        and overwritten. lr is a Python number or a one-element float32 device tensor, read by the kernel at every call.
        max_grad_norm None = no clipping. The hyperparameters reach the kernel as float32. The workspace (one per total size) and
        the filled argument block (one per set of addresses) are the engine's. Returns `state`; nothing synchronises."""
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
            if not torch.is_tensor(p) or not torch.is_tensor(g):
                raise ValueError(f"params[{i}] and grads[{i}] must be tensors, got {type(p).__name__} and {type(g).__name__}")
            self._check_f32(g, tuple(p.shape), f"grads[{i}]")
        key = tuple(t.data_ptr() for ts in lists.values() for t in ts) + (state.data_ptr() if torch.is_tensor(state) else None,
                                                                          None if lr_dev is None else lr_dev.data_ptr())
        cache = self.__dict__.setdefault("_adam", {})
        o = cache.get(key)
        if o is None:
            for i, p in enumerate(params):
                self._check_f32(p, tuple(p.shape), f"params[{i}]")
                for name in ("exp_avg", "exp_avg_sq"):
                    if not torch.is_tensor(lists[name][i]):
                        raise ValueError(f"{name}[{i}] must be a tensor, got {type(lists[name][i]).__name__}")
                    self._check_f32(lists[name][i], tuple(p.shape), f"{name}[{i}]")
                if p.numel() < 1:
                    raise ValueError(f"params[{i}] must hold at least one element, got shape {tuple(p.shape)}")
            if not torch.is_tensor(state):
                raise ValueError(f"state must be a float64 tensor of shape (8,), got {type(state).__name__}")
            self._check(state, (8,), (torch.float64,), "state")
            if lr_dev is not None:
                self._check_f32(lr_dev, tuple(lr_dev.shape) if lr_dev.numel() == 1 else (1,), "lr")
            total = sum(p.numel() for p in params)
            nbytes = int(self.lib.pf_adam_workspace_bytes(total))
            if nbytes < 1:
                raise ValueError(f"params: the total number of elements must be below 2^31, got {total}")
            spaces = self.__dict__.setdefault("_adam_ws", {})
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
        for name, x in (("eps", eps), ("weight_decay", weight_decay)) + (() if lr_dev is not None else (("lr", lr),)) \
                + (() if max_grad_norm is None else (("max_grad_norm", max_grad_norm),)):
            if isinstance(x, bool) or not isinstance(x, (int, float)):
                raise ValueError(f"{name} must be a Python number" + (" or a one-element float32 device tensor" if name == "lr" else "") + f", got {type(x).__name__}")
        try:
            b1, b2 = betas
            b1, b2 = float(b1), float(b2)
        except (TypeError, ValueError):
            raise ValueError(f"betas must be a pair of numbers, got {betas!r}") from None
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"betas must lie in [0, 1), got {betas!r}")
        if lr_dev is None and not 0.0 <= float(lr) < float("inf"):
            raise ValueError(f"lr must be finite and >= 0, got {lr}")
        if not 0.0 < float(eps) < float("inf"):
            raise ValueError(f"eps must be finite and > 0, got {eps}")
        if not 0.0 <= float(weight_decay) < float("inf"):
            raise ValueError(f"weight_decay must be finite and >= 0, got {weight_decay}")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError(f"max_grad_norm must be > 0 or None (no clipping), got {max_grad_norm}")
        if not isinstance(skip_nonfinite, bool):
            raise ValueError(f"skip_nonfinite must be a bool, got {type(skip_nonfinite).__name__}")
        a = o["args"]
        a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = (0.0 if lr_dev is not None else float(lr)), b1, b2, float(eps), float(weight_decay)
        a.max_grad_norm, a.skip_nonfinite = (float("inf") if max_grad_norm is None else float(max_grad_norm)), int(skip_nonfinite)
        with torch.cuda.device(self.device):
            L.check(self.lib.pf_adam_step(self._ctx, o["ref"], o["workspace"], o["bytes"], C.c_void_p(_raw_stream(self._index))), self._ctx)
        return state

    def body_tick(self, wrench, n_ticks: int = 1):
        """pf_body_tick: the free-body tick alone under a held body-frame wrench [n, 6] (force, torque)."""
        self._aviary_outputs()
        self._check_f32(wrench, (self.n, 6), "wrench")
        b = self._buffers(wrench=wrench)
        with torch.cuda.device(self.device):
            L.check(self.lib.pf_body_tick(self._ctx, C.byref(b), int(n_ticks), self._stream()), self._ctx)
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
        self._check_f32(start_pose, (self.n, 7), "start_pose")
        self._check_per_lane()
        b = self._buffers(start_pose=start_pose)
        with torch.cuda.device(self.device):
            L.check(self.lib.pf_aviary_reset(self._ctx, C.byref(b), self._stream()), self._ctx)
        self.params.flight_mode = 0

    def aviary_set_mode(self, mode: int, setpoints):
        self._aviary_outputs()
        self._check_f32(setpoints, (self.n, self._sp_dim(int(mode))), "setpoints")
        self._check_per_lane()
        b = self._buffers()
        with torch.cuda.device(self.device):
            L.check(self.lib.pf_aviary_set_mode(self._ctx, C.byref(b), int(mode), _ptr(setpoints), self._stream()), self._ctx)
        self.params.flight_mode = int(mode)

    def aviary_step(self, setpoints, n_steps: int = 1, xi=None):
        self._aviary_outputs()
        self._check_f32(setpoints, (self.n, self._sp_dim()), "setpoints")
        self._check_f32(xi, (int(n_steps) * self.params.ticks_per_control, self.n), "xi")
        self._check_per_lane()
        b = self._buffers(setpoints=setpoints, xi=xi)
        with torch.cuda.device(self.device):
            L.check(self.lib.pf_aviary_step(self._ctx, C.byref(b), int(n_steps), self._stream()), self._ctx)
        return self.out_state, self.out_aux

    def aviary_tick(self, setpoints, tick_index: int, wind=None, xi=None):
        """One physics tick of Aviary.step (pf_aviary_tick). `wind`: [n, wind_links, 3] world-frame wind
        as sampled after the previous tick, or None. Fills out_state / out_aux / out_contact (this
        tick's contact verdict) / link_pos (where to sample the field next)."""
        self._aviary_outputs()
        self._check_f32(wind, (self.n, self.wind_links, 3), "wind")
        self._check_f32(xi, (self.n,), "xi")
        self._check_f32(setpoints, (self.n, self._sp_dim()), "setpoints")
        self._check_per_lane()
        b = self._buffers(setpoints=setpoints, xi=xi, wind=wind)
        with torch.cuda.device(self.device):
            L.check(self.lib.pf_aviary_tick(self._ctx, C.byref(b), int(tick_index), self._stream()), self._ctx)
        return self.out_state, self.out_aux

    # ------------------------------------------------------------------ state views
    def ints(self):
        """[n, 4] int32 view: step_count, flags, rng_ctr, n_targets_left."""
        g = 5 if self.params.vehicle == L.FIXEDWING else 6
        return self.state[g].view(torch.int32)

    def flags(self):
        return self.ints()[:, 1]

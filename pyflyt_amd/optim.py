"""pf_adam_step behind torch.optim.Adam's interface: Adam / AdamW with global gradient-norm clipping over a model's parameters in two
launches, the step counter and (optionally) the learning rate on the device (BatchEngine.adam_step; include/pyflyt_amd.h has the
semantics). With pyflyt_amd.mlp and pyflyt_amd.ppo_loss in front of it, an epoch holds no torch arithmetic and is capturable whole."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L

STATE_SLOTS = ("step", "grad_norm", "clip_coef", "lr", "skipped")
KL_LR_KEYS = ("factor", "low", "high", "min", "max")


def _f32(x):
    return C.c_float(float(x)).value


class Adam:
    """opt = Adam(env, params, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None, skip_nonfinite=False)

    `params`: up to 32 contiguous float32 tensors on the engine's device (torch.nn.Parameters as they are), updated in place -- an
    MLPPolicy.from_torch over them sees the step at the next rollout. One group: a list of dicts is refused. weight_decay is
    decoupled (AdamW); max_grad_norm clips the global gradient norm as torch.nn.utils.clip_grad_norm_ does, without writing the
    gradients; skip_nonfinite leaves everything as it was where that norm is not finite (and counts the call). `lr` is a Python
    number, or a one-element float32 device tensor that the kernel reads at every step: what a captured epoch anneals.

    The hyperparameters reach the kernel as float32 and are held here as those values: `betas` reads (0.8999999762, 0.9990000129)
    after betas=(0.9, 0.999). There is ONE step counter for all parameters (state[0]): a parameter that sat out steps because its
    .grad was None is bias-corrected with the common counter, where torch counts per parameter.

    target_kl (None: off, and nothing below applies) puts the KL decisions of a PPO recipe on the device: step(stats=...) is then
    pf_kl_control followed by pf_adam_step_gated, and the step is taken only where stats' approx_kl <= kl_stop * target_kl (kl_stop
    >= 1; inf: never stop). Once a step has pushed the KL over that limit the later epochs on the same batch measure the same KL and
    are skipped too: early stopping without a host read. kl_lr = dict(factor=, low=, high=, min=, max=) adapts the learning rate
    in the same launch (lr / factor where kl > high * target_kl, lr * factor where kl < low * target_kl, within [min, max]); it needs
    `lr` to be a device tensor. kl_dict() reads what was decided."""

    def __init__(self, env_or_engine, params, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None, skip_nonfinite=False,
                 target_kl=None, kl_stop=1.5, kl_lr=None):
        engine = getattr(env_or_engine, "engine", env_or_engine)
        if not hasattr(engine, "adam_step"):
            raise ValueError(f"the first argument must be a vector env or a BatchEngine, got {type(env_or_engine).__name__}")
        try:
            params = list(params)
        except TypeError:
            raise ValueError(f"params must be an iterable of tensors, got {type(params).__name__}") from None
        if any(isinstance(p, dict) for p in params):
            raise ValueError("params: per-group hyperparameters are not supported (there is one group): pass the tensors themselves, not a list of dicts")
        if not 1 <= len(params) <= L.PF_ADAM_MAX_TENSORS:
            raise ValueError(f"params: 1..{L.PF_ADAM_MAX_TENSORS} tensors (PF_ADAM_MAX_TENSORS), got {len(params)}")
        for i, p in enumerate(params):
            if not torch.is_tensor(p):
                raise ValueError(f"params[{i}] must be a tensor, got {type(p).__name__}")
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != engine.device or p.numel() < 1:
                raise ValueError(f"params[{i}] must be a contiguous float32 tensor with at least one element on {engine.device}, "
                                 f"got {p.dtype} {tuple(p.shape)} on {p.device}" + ("" if p.is_contiguous() else " (not contiguous)"))
            for j in range(i):
                if params[j] is p or params[j].data_ptr() == p.data_ptr():
                    raise ValueError(f"params[{i}] is the same tensor as params[{j}]: a parameter may be given once")
        self.engine, self.params = engine, params
        self.exp_avg = [torch.zeros_like(p, memory_format=torch.contiguous_format).detach() for p in params]
        self.exp_avg_sq = [torch.zeros_like(p, memory_format=torch.contiguous_format).detach() for p in params]
        self.state = torch.zeros(8, dtype=torch.float64, device=engine.device)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.target_kl, self.kl_stop, self.kl_lr = None, float("inf"), None
        if target_kl is None:
            if kl_lr is not None:
                raise ValueError("kl_lr comes with target_kl (the KL its thresholds are multiples of)")
            return
        num = (int, float)
        if isinstance(target_kl, bool) or not isinstance(target_kl, num) or not 0.0 < float(target_kl) < float("inf"):
            raise ValueError(f"target_kl must be None or a finite Python number > 0, got {target_kl!r}")
        if isinstance(kl_stop, bool) or not isinstance(kl_stop, num) or not float(kl_stop) >= 1.0:
            raise ValueError(f"kl_stop must be a Python number >= 1 (inf: never stop), got {kl_stop!r}")
        if kl_lr is not None:
            if not isinstance(kl_lr, dict) or sorted(kl_lr) != sorted(KL_LR_KEYS):
                raise ValueError(f"kl_lr must be a dict with the keys {KL_LR_KEYS}, got {kl_lr!r}")
            if any(isinstance(v, bool) or not isinstance(v, num) or not 0.0 < float(v) < float("inf") for v in kl_lr.values()):
                raise ValueError(f"kl_lr: every value must be a finite Python number > 0, got {kl_lr!r}")
            if not (kl_lr["factor"] > 1.0 and kl_lr["low"] < kl_lr["high"] and kl_lr["min"] <= kl_lr["max"]):
                raise ValueError(f"kl_lr needs factor > 1, low < high and min <= max, got {kl_lr!r}")
            if not torch.is_tensor(self._lr):
                raise ValueError("kl_lr changes the learning rate on the device: lr must be a one-element float32 device tensor")
            self.kl_lr = {k: _f32(kl_lr[k]) for k in KL_LR_KEYS}
        self.target_kl, self.kl_stop = _f32(target_kl), _f32(kl_stop)
        self.gate = torch.ones(1, dtype=torch.int32, device=engine.device)
        self.kl_state = torch.zeros(4, dtype=torch.float64, device=engine.device)

    # ------------------------------------------------------------------ hyperparameters, as the float32 values the kernel applies
    @property
    def lr(self):
        return self._lr

    @lr.setter
    def lr(self, value):
        if torch.is_tensor(value):
            if value.dtype != torch.float32 or value.numel() != 1 or value.device != self.engine.device:
                raise ValueError(f"lr must be a Python number or a one-element float32 tensor on {self.engine.device}, got {value.dtype} {tuple(value.shape)} on {value.device}")
            self._lr = value
        else:
            if isinstance(value, bool) or not isinstance(value, (int, float)) or not 0.0 <= float(value) < float("inf"):
                raise ValueError(f"lr must be a finite Python number >= 0 or a one-element float32 device tensor, got {value!r}")
            self._lr = _f32(value)

    @property
    def betas(self):
        return self._betas

    @betas.setter
    def betas(self, value):
        try:
            b1, b2 = (_f32(b) for b in value)
        except (TypeError, ValueError):
            raise ValueError(f"betas must be a pair of numbers, got {value!r}") from None
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"betas must lie in [0, 1) as float32, got {value!r}")
        self._betas = (b1, b2)

    @property
    def eps(self):
        return self._eps

    @eps.setter
    def eps(self, value):
        if not 0.0 < _f32(value) < float("inf"):
            raise ValueError(f"eps must be finite and > 0 as float32, got {value!r}")
        self._eps = _f32(value)

    @property
    def weight_decay(self):
        return self._weight_decay

    @weight_decay.setter
    def weight_decay(self, value):
        if not 0.0 <= _f32(value) < float("inf"):
            raise ValueError(f"weight_decay must be finite and >= 0, got {value!r}")
        self._weight_decay = _f32(value)

    # ------------------------------------------------------------------ the step
    def step(self, grads=None, stats=None, adapt_lr=True):
        """One step. Without `grads`, every parameter's .grad; parameters whose .grad is None take no part, neither in the norm nor in
        the update (none at all: nothing happens). With `grads`, a list of one gradient tensor per parameter, e.g.
        engine.mlp_backward's own tensors. With target_kl, `stats` (the [16] block of the ppo_loss / ppo_grad call that made the
        gradients) is required: its approx_kl decides on the device whether the step is taken, and with kl_lr and adapt_lr the new
        learning rate (adapt_lr=False: not in this call -- a recipe adapts once per batch, on its last epoch). Returns nothing and
        synchronises nothing."""
        if self.target_kl is None:
            if stats is not None:
                raise ValueError("stats is read only with target_kl (this optimiser has none)")
        elif stats is None:
            raise ValueError("stats (the [16] block of ppo_loss / ppo_grad) is required with target_kl")
        if grads is None:
            live = [i for i, p in enumerate(self.params) if p.grad is not None]
            if not live:
                return
            if len(live) == len(self.params):
                params, m, v = self.params, self.exp_avg, self.exp_avg_sq
            else:
                params, m, v = [self.params[i] for i in live], [self.exp_avg[i] for i in live], [self.exp_avg_sq[i] for i in live]
            grads = [p.grad for p in params]
        else:
            grads = list(grads)
            if len(grads) != len(self.params):
                raise ValueError(f"grads must hold one tensor per parameter ({len(self.params)}), got {len(grads)}")
            params, m, v = self.params, self.exp_avg, self.exp_avg_sq
        gate = None
        if self.target_kl is not None:
            adapt = bool(adapt_lr) and self.kl_lr is not None
            lr_args = dict(factor=self.kl_lr["factor"], low=self.kl_lr["low"], high=self.kl_lr["high"], lr_min=self.kl_lr["min"], lr_max=self.kl_lr["max"]) if adapt else {}
            gate = self.gate
            self.engine.kl_control(stats, gate, self.kl_state, self.target_kl, self.kl_stop, lr=self._lr if torch.is_tensor(self._lr) else None, adapt=adapt, **lr_args)
        self.engine.adam_step(params, grads, m, v, self.state, lr=self._lr, betas=self._betas, eps=self._eps, weight_decay=self._weight_decay,
                              max_grad_norm=self.max_grad_norm, skip_nonfinite=self.skip_nonfinite, gate=gate)

    def zero_grad(self, set_to_none: bool = True):
        for p in self.params:
            if p.grad is None:
                continue
            if set_to_none:
                p.grad = None
            else:
                p.grad.detach_()
                p.grad.requires_grad_(False)
                p.grad.zero_()

    def stats_dict(self):
        """{step, grad_norm (before clipping), clip_coef, lr, skipped} of the last step, as Python numbers: the one host synchronisation."""
        s = self.state.tolist()
        return dict(zip(STATE_SLOTS, [int(s[0]), s[1], s[2], s[3], int(s[4])]))

    def kl_dict(self):
        """{approx_kl, lr, gate, gated_calls (gates the control closed), gated_steps (steps the optimiser skipped for a closed gate)}
        of the last step with target_kl, as Python numbers. Synchronises."""
        if self.target_kl is None:
            raise ValueError("kl_dict() needs an optimiser made with target_kl")
        k, gated = self.kl_state.tolist(), float(self.state[5])
        return dict(approx_kl=k[0], lr=k[1], gate=int(k[2]), gated_calls=int(k[3]), gated_steps=int(gated))

    # ------------------------------------------------------------------ checkpoints in torch.optim.Adam's layout
    def _torch_group(self):
        lr = float(self._lr) if torch.is_tensor(self._lr) else self._lr
        group = dict(torch.optim.Adam([torch.zeros(1)], lr=lr, betas=self._betas, eps=self._eps, weight_decay=self._weight_decay).param_groups[0])
        if "decoupled_weight_decay" in group:
            group["decoupled_weight_decay"] = self._weight_decay > 0.0
        group["params"] = list(range(len(self.params)))
        return group

    def state_dict(self):
        """torch.optim.Adam's layout: state[i] = {step, exp_avg, exp_avg_sq} (copies) and one param_group, so that
        torch.optim.Adam / AdamW .load_state_dict takes it (AdamW where weight_decay > 0: the decay here is decoupled). Synchronises."""
        step = float(self.state[0])
        state = {}
        if step > 0:
            for i in range(len(self.params)):
                state[i] = dict(step=torch.tensor(step, dtype=torch.float32), exp_avg=self.exp_avg[i].clone(), exp_avg_sq=self.exp_avg_sq[i].clone())
        sd = dict(state=state, param_groups=[self._torch_group()])
        if self.target_kl is not None:  # (a key torch's optimisers ignore)
            sd["kl_control"] = dict(state=self.kl_state.tolist(), gate=int(self.gate), gated_steps=float(self.state[5]))
        return sd

    def load_state_dict(self, sd):
        """Takes this class's state_dict() or torch.optim.Adam's / AdamW's over the same parameters in the same order."""
        groups = sd["param_groups"]
        if len(groups) != 1:
            raise ValueError(f"param_groups: there is one group here, the checkpoint has {len(groups)}")
        g = groups[0]
        if len(g["params"]) != len(self.params):
            raise ValueError(f"param_groups[0].params: {len(g['params'])} parameters in the checkpoint, {len(self.params)} here")
        if g.get("amsgrad") or g.get("maximize"):
            raise ValueError("param_groups[0]: amsgrad and maximize are not supported")
        state = {k: sd["state"][pid] for k, pid in enumerate(g["params"]) if pid in sd["state"]}
        if state and len(state) != len(self.params):
            raise ValueError(f"state: {len(state)} of {len(self.params)} parameters have optimiser state; there is one step counter for all of them")
        steps = {float(s["step"]) for s in state.values()}
        if len(steps) > 1:
            raise ValueError(f"state: the parameters' step counts differ ({sorted(steps)}); there is one step counter for all of them")
        for i, s in state.items():
            if s.get("max_exp_avg_sq") is not None:
                raise ValueError(f"state[{i}]: amsgrad is not supported")
            if tuple(s["exp_avg"].shape) != tuple(self.params[i].shape) or tuple(s["exp_avg_sq"].shape) != tuple(self.params[i].shape):
                raise ValueError(f"state[{i}]: exp_avg / exp_avg_sq must have the parameter's shape {tuple(self.params[i].shape)}")
        self.betas, self.eps, self.weight_decay = g["betas"], g["eps"], g["weight_decay"]
        lr = float(g["lr"])
        if torch.is_tensor(self._lr):
            self._lr.fill_(lr)
        else:
            self.lr = lr
        for i in range(len(self.params)):
            if i in state:
                self.exp_avg[i].copy_(state[i]["exp_avg"])
                self.exp_avg_sq[i].copy_(state[i]["exp_avg_sq"])
            else:
                self.exp_avg[i].zero_()
                self.exp_avg_sq[i].zero_()
        self.state.zero_()
        self.state[0] = steps.pop() if steps else 0.0
        kl = sd.get("kl_control")
        if self.target_kl is not None:
            self.kl_state.copy_(torch.tensor(kl["state"] if kl else [0.0] * 4, dtype=torch.float64))
            self.gate.fill_(kl["gate"] if kl else 1)
            self.state[5] = kl["gated_steps"] if kl else 0.0

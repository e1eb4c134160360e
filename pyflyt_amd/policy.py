"""MLPPolicy: the small policy network that BatchEngine.rollout_policy evaluates on the device, per lane, between two env steps of
one launch (pf_rollout_policy, include/pyflyt_amd.h), and that BatchEngine.policy_act evaluates for all lanes in a launch of its own
(pf_policy_act: every env, action widths 4, 6 and 7).

The policy HOLDS REFERENCES to the parameter tensors it is given, not copies: the library reads them at every rollout, so an
optimiser step that updates them in place is seen by the next rollout without any call. The one exception is observation
normalisation: `obs_mean` / `obs_std` are folded into the first layer on the host (W' = W / std, b' = b - W' mean), and the folded
tensors are copies -- call refresh() after the first layer or the statistics have changed.
"""
from __future__ import annotations

import torch

from . import _lib as L

MAX_HIDDEN = L._DEFINES["PF_POLICY_MAX_HIDDEN"]
_ACTIVATIONS = {"tanh": L._ENUMS["PF_ACT_TANH"], "relu": L._ENUMS["PF_ACT_RELU"]}


def _check_param(t, name, ndim):
    if not torch.is_tensor(t):
        raise ValueError(f"{name} must be a torch tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")
    if t.dim() != ndim:
        raise ValueError(f"{name} must have {ndim} dimension(s), got shape {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous (the kernel reads torch.nn.Linear's row-major layout); got strides {t.stride()}")
    return t


class MLPPolicy:
    """mean = W_L act(... act(W_0 o + b_0) ...) + b_L, action = mean + exp(log_std) * eps.

    layers:      [(weight, bias), ...] in torch.nn.Linear's layout (weight [out, in], bias [out]), float32, contiguous; two or
                 three of them (one or two hidden layers of width 1..64)
    activation:  "tanh" or "relu", on the hidden layers
    log_std:     [action_dim] float32, or None for a deterministic policy (action = mean)
    obs_mean, obs_std: [obs_dim] statistics of an observation normaliser, folded into the first layer (see the module docstring)
    """

    def __init__(self, layers, activation="tanh", log_std=None, obs_mean=None, obs_std=None):
        layers = [tuple(l) for l in layers]
        if len(layers) not in (2, 3):
            raise ValueError(f"layers: a policy has 2 or 3 affine layers (1 or 2 hidden layers), got {len(layers)}")
        if activation not in _ACTIVATIONS:
            raise ValueError(f"activation must be 'tanh' or 'relu', got {activation!r}")
        for l, (w, b) in enumerate(layers):
            _check_param(w, f"layers[{l}].weight", 2)
            _check_param(b, f"layers[{l}].bias", 1)
            if b.shape[0] != w.shape[0]:
                raise ValueError(f"layers[{l}].bias has {b.shape[0]} entries for a weight of {w.shape[0]} rows")
            if l > 0 and w.shape[1] != layers[l - 1][0].shape[0]:
                raise ValueError(f"layers[{l}].weight reads {w.shape[1]} inputs, layers[{l - 1}] writes {layers[l - 1][0].shape[0]}")
            if l + 1 < len(layers) and not 1 <= w.shape[0] <= MAX_HIDDEN:
                raise ValueError(f"layers[{l}].weight: hidden width {w.shape[0]} is outside 1..{MAX_HIDDEN} (PF_POLICY_MAX_HIDDEN)")
            if w.device != layers[0][0].device or b.device != w.device:
                raise ValueError(f"layers[{l}]: every parameter must live on one device")
        self.layers = layers
        self.activation = activation
        self.obs_dim = int(layers[0][0].shape[1])
        self.action_dim = int(layers[-1][0].shape[0])
        self.widths = [int(w.shape[0]) for w, _ in layers[:-1]]
        if log_std is not None:
            _check_param(log_std, "log_std", 1)
            if log_std.shape[0] != self.action_dim:
                raise ValueError(f"log_std has {log_std.shape[0]} entries for an action width of {self.action_dim}")
        self.log_std = log_std
        if (obs_mean is None) != (obs_std is None):
            raise ValueError("obs_mean and obs_std come together")
        for name, t in (("obs_mean", obs_mean), ("obs_std", obs_std)):
            if t is not None:
                _check_param(t, name, 1)
                if t.shape[0] != self.obs_dim:
                    raise ValueError(f"{name} has {t.shape[0]} entries for an observation width of {self.obs_dim}")
        self.obs_mean, self.obs_std = obs_mean, obs_std
        self._first = None
        self.refresh()

    @property
    def device(self):
        return self.layers[0][0].device

    def refresh(self):
        """Recompute the folded first layer (observation normalisation) from the current parameters and statistics. Without
        obs_mean / obs_std there is nothing to refresh: the first layer is read in place like the others."""
        if self.obs_mean is None:
            self._first = self.layers[0]
            return self
        with torch.no_grad():
            w, b = self.layers[0]
            wf = (w / self.obs_std.to(w.device)[None, :]).contiguous()
            bf = (b - wf @ self.obs_mean.to(w.device)).contiguous()
        self._first = (wf, bf)
        return self

    def set_obs_stats(self, mean, std):
        """The statistics of the observation normaliser, e.g. env.obs_rms.mean and env.obs_rms.std() after a collect(stats=True):
        copied into obs_mean / obs_std (created on the first layer's device if the policy had none), then refresh()."""
        for name, t in (("mean", mean), ("std", std)):
            _check_param(t, name, 1)
            if t.shape[0] != self.obs_dim:
                raise ValueError(f"{name} has {t.shape[0]} entries for an observation width of {self.obs_dim}")
        if self.obs_mean is None:
            self.obs_mean, self.obs_std = torch.empty(self.obs_dim, device=self.device), torch.empty(self.obs_dim, device=self.device)
        with torch.no_grad():
            self.obs_mean.copy_(mean)
            self.obs_std.copy_(std)
        return self.refresh()

    def device_layers(self):
        """The (weight, bias) tensors the kernel reads: the folded first layer, then the others as given."""
        return [self._first] + self.layers[1:]

    @classmethod
    def from_torch(cls, seq, log_std=None, obs_mean=None, obs_std=None):
        """From a torch.nn.Sequential of Linear layers with ONE kind of activation (Tanh or ReLU) between them. The policy refers to
        the modules' parameter tensors (`.data` shares their storage)."""
        nn = torch.nn
        if not isinstance(seq, nn.Sequential):
            raise ValueError(f"from_torch takes a torch.nn.Sequential, got {type(seq).__name__}")
        mods = list(seq)
        layers, acts = [], set()
        for i, m in enumerate(mods):
            if i % 2 == 0:
                if not isinstance(m, nn.Linear):
                    raise ValueError(f"from_torch: module {i} must be a Linear, got {type(m).__name__}")
                if m.bias is None:
                    raise ValueError(f"from_torch: module {i} (Linear) has no bias")
                layers.append((m.weight.data, m.bias.data))
            else:
                if not isinstance(m, (nn.Tanh, nn.ReLU)):
                    raise ValueError(f"from_torch: module {i} must be a Tanh or a ReLU, got {type(m).__name__}")
                acts.add("tanh" if isinstance(m, nn.Tanh) else "relu")
        if len(mods) % 2 == 0:
            raise ValueError("from_torch: the Sequential must end with a Linear (the output layer is affine)")
        if len(acts) > 1:
            raise ValueError("from_torch: one kind of activation per policy (Tanh or ReLU), got both")
        if isinstance(log_std, nn.Parameter):
            log_std = log_std.data
        return cls(layers, activation=(acts.pop() if acts else "tanh"), log_std=log_std, obs_mean=obs_mean, obs_std=obs_std)

    def forward_reference(self, obs, dtype=torch.float64):
        """The same network in plain torch, in `dtype`, from the tensors the kernel reads (tests, debugging): the mean."""
        h = obs.to(dtype)
        ls = self.device_layers()
        for l, (w, b) in enumerate(ls):
            h = h @ w.to(device=h.device, dtype=dtype).T + b.to(device=h.device, dtype=dtype)
            if l + 1 < len(ls):
                h = torch.tanh(h) if self.activation == "tanh" else torch.relu(h)
        return h

    def fill(self, q, engine):
        """Fill a pf_policy block for `engine` (checks the widths against the engine's observation and action widths and the device)."""
        if self.obs_dim != engine.obs_dim:
            raise ValueError(f"layers[0].weight reads {self.obs_dim} inputs, the env observes {engine.obs_dim}")
        if self.action_dim != engine.action_dim:
            raise ValueError(f"the last layer writes {self.action_dim} outputs, the env's action width is {engine.action_dim}")
        ls = self.device_layers()
        for t in [x for wb in ls for x in wb] + ([self.log_std] if self.log_std is not None else []):
            if t.device != engine.device:
                raise ValueError(f"policy parameters must live on {engine.device}, got {t.device}")
        q.n_layers = len(ls)
        q.activation = _ACTIVATIONS[self.activation]
        for l in range(2):
            q.width[l] = self.widths[l] if l < len(self.widths) else 0
        for l in range(3):
            q.w[l] = ls[l][0].data_ptr() if l < len(ls) else None
            q.b[l] = ls[l][1].data_ptr() if l < len(ls) else None
        q.log_std = self.log_std.data_ptr() if self.log_std is not None else None
        return q

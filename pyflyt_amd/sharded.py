"""One PPO gradient from shards of a batch that live on several devices (include/pyflyt_amd.h: SHARDED PPO).
One process, one engine and one stream per device, no collective: what crosses devices are torch copies of 4 doubles, 24 doubles and
one flat gradient buffer per shard, and torch orders the streams around them. Replicas keeps the networks' copies; ppo_grad_sharded
is ppo_grad for a list of shards."""
from __future__ import annotations

import torch

from .ppo import _batch_tensors, _options


def _leaves(obj, name):
    """The tensors of a module or of a bare tensor / Parameter, in a fixed order."""
    if isinstance(obj, torch.nn.Module):
        return list(obj.parameters()) + list(obj.buffers())
    if torch.is_tensor(obj):
        return [obj]
    raise ValueError(f"modules[{name!r}] must be a torch.nn.Module or a tensor, got {type(obj).__name__}")


class Replicas:
    """rep = Replicas(dict(actor=actor, critic=critic, log_std=log_std), devices): the master modules / parameters live on devices[0]
    (and are what the optimiser steps); every further device gets a copy. rep[g] is the dict for device g -- the master's own where
    that device is devices[0]. rep.sync() copies master -> copies with copy_(non_blocking=True): call it after the optimiser's step.
    ppo_grad_sharded reads the keys "actor", "critic" and "log_std"."""

    def __init__(self, modules, devices):
        import copy

        if not isinstance(modules, dict) or not modules:
            raise ValueError(f"modules must be a non-empty dict of torch.nn.Modules / tensors by name, got {type(modules).__name__}")
        try:
            self.devices = [torch.device(d) for d in devices]
        except TypeError:
            raise ValueError(f"devices must be a list of devices, got {type(devices).__name__}") from None
        if not self.devices:
            raise ValueError("devices must name at least one device")
        for name, obj in modules.items():
            for t in _leaves(obj, name):
                if t.device != self.devices[0]:
                    raise ValueError(f"modules[{name!r}] must live on devices[0] ({self.devices[0]}), got a tensor on {t.device}")
        self.master = dict(modules)
        self._dicts, self._pairs = [], []  # per device: the dict; [(master tensor, copy)] of the devices that hold copies
        for d in self.devices:
            if d == self.devices[0]:
                self._dicts.append(self.master)
                continue
            made = {}
            for name, obj in modules.items():
                if isinstance(obj, torch.nn.Module):
                    made[name] = copy.deepcopy(obj).to(d)
                else:
                    made[name] = obj.detach().to(d, copy=True)
                self._pairs += list(zip(_leaves(obj, name), _leaves(made[name], name)))
            self._dicts.append(made)
        self._grad = None  # ppo_grad_sharded's flat gradient of the master parameters, made at first use

    def __len__(self):
        return len(self.devices)

    def __getitem__(self, g):
        return self._dicts[g]

    @torch.no_grad()
    def sync(self):
        """master -> every copy, enqueued; nothing waits for the host."""
        for src, dst in self._pairs:
            dst.copy_(src, non_blocking=True)


def ppo_grad_sharded(env, xs, rep, batches, *, rows=None, valid=None, clip: float = 0.2, vf_coef: float = 0.5, ent_coef: float = 0.0,
                     normalize_advantage: bool = True, activation=None, clip_vf=None, action_bounds=None, bounds_coef: float = 0.0):
    """stats = ppo_grad_sharded(env, xs, rep, batches): ppo_grad for ONE batch that lies in shards, one per entry of env.shards (a
    ShardedVecEnv, or a list of vector envs / BatchEngines), of xs (the networks' inputs, [rows_g, in_dim] each) and of batches (the
    dicts collect returned, or 4-tuples (actions, logp_old, advantages, returns) with valid= a list). rows: None, or a list of int32
    index lists, one per shard (an entry may be None). The advantages are normalised and the rows weighted over ALL shards' valid
    rows: the result is the gradient of the joint batch, not a sum of per-shard gradients.

    Per shard, on its device: ppo_adv_sums; the 4 doubles go to devices[0], are added there (pf_adv_sums_add) and come back;
    ppo_grad_shard with rep[g]'s networks; its flat gradient and block go to devices[0], where ppo_shard_combine adds them up in
    shard order. The gradients are LEFT in .grad of the master parameters (rep[0]) as views of one flat buffer that rep owns,
    overwritten by the next call -- assigned, not accumulated. Returns stats [16] float64 on devices[0] (a copy): Adam.step(stats=)
    and ppo_stats_dict take it as they take ppo_grad's. The copies are torch's, so torch orders the streams; nothing here
    synchronises with the host."""
    from .nets import parse_net

    shards = list(getattr(env, "shards", env))
    engines = [getattr(s, "engine", s) for s in shards]
    G = len(engines)
    if not isinstance(rep, Replicas):
        raise ValueError(f"rep must be a Replicas, got {type(rep).__name__}")
    for name, v in (("xs", xs), ("batches", batches), ("rows", rows), ("valid", valid)):
        if v is not None and (not isinstance(v, (list, tuple)) or len(v) != G):
            raise ValueError(f"{name} must be a list with one entry per shard ({G}), got {len(v) if isinstance(v, (list, tuple)) else type(v).__name__}")
    if xs is None or batches is None:
        raise ValueError("xs and batches are required: lists with one entry per shard")
    if len(rep) != G:
        raise ValueError(f"rep holds {len(rep)} devices, the env {G} shards: one replica per shard")
    for g, e in enumerate(engines):
        if not hasattr(e, "ppo_grad_shard"):
            raise ValueError(f"shards[{g}] must be a vector env or a BatchEngine, got {type(shards[g]).__name__}")
        if e.device != rep.devices[g]:
            raise ValueError(f"shards[{g}] lives on {e.device}, rep[{g}] on {rep.devices[g]}")
    missing = [k for k in ("actor", "critic", "log_std") if k not in rep.master]
    if missing:
        raise ValueError(f"rep lacks {missing}: ppo_grad_sharded reads the keys 'actor', 'critic' and 'log_std'")
    dev0, eng0 = rep.devices[0], engines[0]

    calls = []  # per shard: what ppo_grad_shard takes
    for g in range(G):
        nets = rep[g]
        a_layers, a_act = parse_net(nets["actor"], activation, "actor")
        c_layers, c_act = parse_net(nets["critic"], activation, "critic")
        x, batch = xs[g], (batches[g],) if isinstance(batches[g], dict) else tuple(batches[g])
        actions, logp_old, advantages, returns, vld, from_dict = _batch_tensors(batch, None if valid is None else valid[g])
        options = _options(batch, clip_vf, action_bounds, bounds_coef, None)
        if from_dict:
            A = actions.shape[-1]
            actions, logp_old, advantages, returns = actions.reshape(-1, A), logp_old.reshape(-1), advantages.reshape(-1), returns.reshape(-1)
            vld = None if vld is None else vld.reshape(-1)
            x = x.reshape(-1, x.shape[-1])
        detached = [[(w.detach(), b.detach()) for w, b in layers] for layers in (a_layers, c_layers)]
        calls.append(dict(x=x, actor=detached[0], critic=detached[1], log_std=nets["log_std"].detach(), actions=actions, logp_old=logp_old,
                          advantages=advantages, returns=returns, valid=vld, clip=clip, vf_coef=vf_coef, ent_coef=ent_coef,
                          normalize_advantage=normalize_advantage, actor_activation=a_act, critic_activation=c_act,
                          rows=None if rows is None else rows[g], **options))
        o = dict(dict(clip_vf=None, action_bounds=None, bounds_coef=0.0, values_old=None), **options)
        c = calls[-1]  # (every shard's refusals before any shard's launch)
        engines[g]._ppo_grad_inputs(c["x"], c["actor"], c["critic"], c["log_std"], actions, logp_old, advantages, returns, vld, clip, vf_coef, ent_coef,
                                    normalize_advantage, a_act, c_act, o["clip_vf"], o["action_bounds"], o["bounds_coef"], o["values_old"], c["rows"])
    # (copy=True: a block that already lies on devices[0] is the engine's own tensor, which its next call overwrites)
    sums = [engines[g].ppo_adv_sums(c["advantages"], valid=c["valid"], rows=c["rows"]).to(dev0, non_blocking=True, copy=True) for g, c in enumerate(calls)]
    total = eng0.adv_sums_add(sums)
    flats, blocks = [], []
    for g, c in enumerate(calls):
        _, _, flat, block = engines[g].ppo_grad_shard(adv_sums=total.to(rep.devices[g], non_blocking=True, copy=True), **c)
        flats.append(flat.to(dev0, non_blocking=True, copy=True))
        blocks.append(block.to(dev0, non_blocking=True, copy=True))
    m_actor, _ = parse_net(rep.master["actor"], activation, "actor")
    m_critic, _ = parse_net(rep.master["critic"], activation, "critic")
    if rep._grad is None or rep._grad.numel() != flats[0].numel():
        rep._grad = torch.empty_like(flats[0])
    grad, gls, stats = eng0.ppo_shard_combine(blocks, total, flats, rep.master["log_std"].detach(), vf_coef=vf_coef, ent_coef=ent_coef,
                                              value_clip=clip_vf is not None, bounds_coef=bounds_coef, out=rep._grad)
    at = 0
    for layers in (m_actor, m_critic):  # (the flat layout of BatchEngine._flat_grads: a network's layers in order, weight then bias)
        for w, b in layers:
            for p in (w, b):
                if p.requires_grad:
                    p.grad = grad[at:at + p.numel()].view(p.shape)
                at += p.numel()
    if rep.master["log_std"].requires_grad:
        rep.master["log_std"].grad = gls
    return stats.clone()

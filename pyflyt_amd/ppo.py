"""pf_ppo_loss behind torch.autograd: the clipped PPO objective as ONE differentiable call between the outputs of the caller's actor
and critic and their output-gradients (BatchEngine.ppo_loss; include/pyflyt_amd.h has the semantics)."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

STAT_NAMES = ("valid_rows", "loss", "policy_loss", "value_loss", "entropy", "approx_kl", "clip_fraction", "advantage_mean", "advantage_std",
              "explained_variance", "ratio_min", "ratio_max")
OPTION_STAT_NAMES = ("value_clip_fraction", "bounds_loss")  # slots 12 and 13, written by the calls with options
ROWS_STAT_NAME = "index_out_of_range"  # slot 14, written by ppo_grad(rows=)


class _PpoLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mean, log_std, value, engine, actions, logp_old, advantages, returns, valid, coefficients):
        gm, gv, gls, stats = engine.ppo_loss(mean.detach().contiguous(), log_std.detach().contiguous(), value.detach().contiguous(), actions, logp_old,
                                             advantages, returns, valid=valid, **coefficients)
        # (the gradients stay in the engine's buffers until backward: the call count tells whether they are still this call's)
        ctx.engine, ctx.calls = engine, engine._ppo_out["calls"]
        ctx.shapes = (mean.shape, value.shape)
        ctx.save_for_backward(gm, gv, gls)
        stats = stats.clone()  # (the engine's block is overwritten by the next call)
        ctx.mark_non_differentiable(stats)
        return stats[1].to(torch.float32), stats

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss, _grad_stats):
        if ctx.engine._ppo_out["calls"] != ctx.calls:
            raise RuntimeError("pyflyt_amd.ppo_loss: backward() came after another ppo_loss call on the same engine, which has overwritten "
                               "this call's gradients; call backward() before the next ppo_loss")
        gm, gv, gls = ctx.saved_tensors
        need = ctx.needs_input_grad
        return (gm.view(ctx.shapes[0]) * grad_loss if need[0] else None, gls * grad_loss if need[1] else None,
                gv.view(ctx.shapes[1]) * grad_loss if need[2] else None, None, None, None, None, None, None, None)


def _options(batch, clip_vf, action_bounds, bounds_coef, values_old):
    """The options of ppo_loss and ppo_grad as the engine's keywords; none at all with the defaults, so that such a call is the one
    it always was. values_old: the batch dict's values, or the explicit tensor."""
    if clip_vf is None and action_bounds is None and values_old is None and isinstance(bounds_coef, (int, float)) and bounds_coef == 0:
        return {}
    if len(batch) == 1 and isinstance(batch[0], dict):
        if values_old is not None:
            raise ValueError("values_old comes from the batch dict (its values); give it only with explicit tensors")
        if clip_vf is not None:
            values_old = batch[0].get("values")
            if values_old is None:
                raise ValueError("the batch lacks ['values'], which clip_vf clips the new values around")
            values_old = values_old.reshape(-1)
    return dict(clip_vf=clip_vf, action_bounds=action_bounds, bounds_coef=bounds_coef, values_old=values_old)


def _batch_tensors(batch, valid):
    """(actions, logp_old, advantages, returns, valid, from_dict) of ppo_loss's and ppo_grad's `*batch`: the dict env.collect
    returned, or the four tensors."""
    if len(batch) == 1 and isinstance(batch[0], dict):
        b = batch[0]
        missing = [k for k in ("actions", "logp", "advantages", "returns") if b.get(k) is None]
        if missing:
            raise ValueError(f"the batch lacks {missing} (env.collect returns logp only for a policy with a log_std)")
        if valid is not None:
            raise ValueError("valid comes from the batch dict; give it only with explicit tensors")
        return b["actions"], b["logp"], b["advantages"], b["returns"], b.get("valid"), True
    if len(batch) == 4:
        return (*batch, valid, False)
    raise ValueError("give the dict env.collect returned, or the four tensors actions, logp_old, advantages, returns")


def ppo_loss(env_or_engine, mean, log_std, value, *batch, valid=None, clip: float = 0.2, vf_coef: float = 0.5, ent_coef: float = 0.0,
             normalize_advantage: bool = True, clip_vf=None, action_bounds=None, bounds_coef: float = 0.0, values_old=None):
    """loss, stats = ppo_loss(env, actor(obs), log_std, critic(obs), batch) with `batch` the dict env.collect returned (its actions,
    logp, advantages, returns and valid, flattened and used whole), or ppo_loss(env, mean, log_std, value, actions, logp_old,
    advantages, returns, valid=...) with explicit tensors such as a gathered minibatch. `loss` is a float32 scalar on the device
    (policy_loss + vf_coef * value_loss - ent_coef * entropy over the valid rows) whose backward() hands mean, log_std and value
    their gradients; `stats` is the [16] float64 device tensor of pf_ppo_loss (ppo_stats_dict names it). Nothing synchronises with
    the host. A deliberate trade: the gradients wait in buffers the engine owns and are NOT copied for backward (a copy would move
    another 40 bytes per row next to a pass of 74), so backward() must come before the next ppo_loss on the same env or engine; a
    later one raises RuntimeError, whatever that next call's shape was, and never uses overwritten gradients. Two losses from one
    engine that are both to be backpropagated need .backward() after each, or an engine each.

    The options (pf_ppo_loss_opt): clip_vf clips the value loss around the batch's values (the dict's, or values_old= with explicit
    tensors); action_bounds=(low, high) with bounds_coef > 0 penalises means outside the box, e.g. env.action_space.low / .high.
    Their gradients come out of the same backward(); ppo_stats_dict(stats, options=True) names their two statistics."""
    engine = getattr(env_or_engine, "engine", env_or_engine)
    if not hasattr(engine, "ppo_loss"):
        raise ValueError(f"the first argument must be a vector env or a BatchEngine, got {type(env_or_engine).__name__}")
    actions, logp_old, advantages, returns, valid, from_dict = _batch_tensors(batch, valid)
    if from_dict:
        mean, value = mean.reshape(actions.shape), value.reshape(advantages.shape)  # ([k n, A] and [k n, 1] from the networks)
    coefficients = dict(clip=clip, vf_coef=vf_coef, ent_coef=ent_coef, normalize_advantage=normalize_advantage,
                        **_options(batch, clip_vf, action_bounds, bounds_coef, values_old))
    if from_dict and coefficients.get("values_old") is not None:
        coefficients["values_old"] = coefficients["values_old"].reshape(advantages.shape)
    return _PpoLoss.apply(mean, log_std, value, engine, actions, logp_old, advantages, returns, valid, coefficients)


def ppo_grad(env_or_engine, x, actor, critic, log_std, *batch, valid=None, clip: float = 0.2, vf_coef: float = 0.5, ent_coef: float = 0.0,
             normalize_advantage: bool = True, activation=None, clip_vf=None, action_bounds=None, bounds_coef: float = 0.0, values_old=None, rows=None):
    """stats = ppo_grad(env, x, actor, critic, log_std, batch): one epoch's gradients in one call (pf_ppo_grad). What
    `ppo_loss(env, mlp(env, x, actor), log_std, mlp(env, x, critic), batch)[0].backward()` leaves in .grad, the network gradients bit
    for bit, without the mean, value and their gradient tensors and without the two forward passes: the tile kernel of the backward
    computes the output layer and the loss's per-row gradients where it used to load them. `actor` and `critic` are what
    pyflyt_amd.mlp accepts (a torch.nn.Sequential, or a list of (weight, bias) with activation=); the critic is one wide; `batch` is
    the dict env.collect returned (flattened and used whole; x then holds its k n rows) or the four tensors actions, logp_old,
    advantages, returns with valid=.

    The gradients are ADDED into .grad of every parameter of the two networks and of log_std (assigned, as copies of the engine's
    tensors, where .grad is None), as loss.backward() does; parameters with requires_grad False are left alone. There is no autograd
    graph and no loss tensor: `stats` is the [16] float64 device tensor of pf_ppo_loss (a copy; ppo_stats_dict names it, slot 1 is
    the loss). x gets no gradient and an x with requires_grad raises ValueError. Nothing synchronises with the host.
    clip_vf, action_bounds, bounds_coef and values_old are ppo_loss's options (pf_ppo_grad_opt).
    rows=idx, a 1-D contiguous int32 device tensor such as one of minibatches(): the call works on the rows of the flattened batch that
    idx names (pf_ppo_grad_rows) and gives what it gives on gathered copies of them, bit for bit, without making the copies; the
    advantages are normalised over those rows. int64 is refused, not converted."""
    from .nets import parse_net

    engine = getattr(env_or_engine, "engine", env_or_engine)
    if not hasattr(engine, "ppo_grad"):
        raise ValueError(f"the first argument must be a vector env or a BatchEngine, got {type(env_or_engine).__name__}")
    a_layers, a_act = parse_net(actor, activation, "actor")
    c_layers, c_act = parse_net(critic, activation, "critic")
    if not torch.is_tensor(x):
        raise ValueError(f"x must be a float32 tensor of shape (..., in_dim), got {type(x).__name__}")
    if x.requires_grad:
        raise ValueError("pyflyt_amd.ppo_grad produces no gradient for x (pf_ppo_grad differentiates the parameters only), and x requires one: "
                         "pass x.detach(), or use torch modules where the input's gradient is needed")
    if not torch.is_tensor(log_std):
        raise ValueError(f"log_std must be a float32 tensor of shape (A,), got {type(log_std).__name__}")
    actions, logp_old, advantages, returns, valid, from_dict = _batch_tensors(batch, valid)
    options = _options(batch, clip_vf, action_bounds, bounds_coef, values_old)
    if from_dict:  # ([k, n, ...] from collect: the rows of x in the same order)
        A = actions.shape[-1]
        actions, logp_old, advantages, returns = actions.reshape(-1, A), logp_old.reshape(-1), advantages.reshape(-1), returns.reshape(-1)
        valid = None if valid is None else valid.reshape(-1)
        x = x.reshape(-1, x.shape[-1])
    detached = [[(w.detach(), b.detach()) for w, b in layers] for layers in (a_layers, c_layers)]
    ga, gc, gls, stats = engine.ppo_grad(x, detached[0], detached[1], log_std.detach(), actions, logp_old, advantages, returns, valid=valid, clip=clip,
                                         vf_coef=vf_coef, ent_coef=ent_coef, normalize_advantage=normalize_advantage, actor_activation=a_act,
                                         critic_activation=c_act, rows=rows, **options)
    pairs = [(p, g) for layers, grads in ((a_layers, ga), (c_layers, gc)) for lp, lg in zip(layers, grads) for p, g in zip(lp, lg)] + [(log_std, gls)]
    for p, g in pairs:  # (the engine owns its tensors and overwrites them at the next call: .grad gets copies, a few KB)
        if not p.requires_grad:
            continue
        if p.grad is None:
            p.grad = g.clone()
        else:
            p.grad.add_(g)
    return stats.clone()


def minibatches(total_rows, n_minibatches, *, device, generator=None):
    """The shuffled minibatches of one epoch over a batch of total_rows rows, as ppo_grad(rows=) takes them: ONE
    torch.randperm(total_rows, dtype=torch.int32) on `device`, cut into n_minibatches contiguous views whose sizes differ by at most
    one (torch.tensor_split). No kernel of this library and no host synchronisation; `generator` (on `device`) makes it repeatable.
    Invalid rows are NOT compacted away: a minibatch names its share of them, the kernels drop them by selection, and w = 1 / c is
    taken per minibatch over its valid rows -- so the minibatches of an epoch weigh the same only as far as their valid counts agree."""
    for name, v in (("total_rows", total_rows), ("n_minibatches", n_minibatches)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"{name} must be an int >= 1, got {v!r}")
    if n_minibatches > total_rows:
        raise ValueError(f"n_minibatches must be at most total_rows ({total_rows}: a minibatch names a row or more), got {n_minibatches}")
    if total_rows >= 2 ** 31 - 64:
        raise ValueError(f"total_rows must be below 2^31 - 64 (the row numbers are int32), got {total_rows}")
    perm = torch.randperm(total_rows, dtype=torch.int32, device=device, generator=generator)
    return list(torch.tensor_split(perm, n_minibatches))


def ppo_stats_dict(stats, options: bool = False, rows: bool = False):
    """The [16] stats tensor of ppo_loss as Python numbers by name (THE place that synchronises with the device); options=True adds
    value_clip_fraction and bounds_loss, the two slots the calls with options write; rows=True adds index_out_of_range, the number
    of slots of a ppo_grad(rows=) call whose row number lay outside the batch (slot 14; 0 after every other call)."""
    values = stats.tolist()
    out = dict(zip(STAT_NAMES + OPTION_STAT_NAMES if options else STAT_NAMES, values))
    out["valid_rows"] = int(out["valid_rows"])
    if rows:
        out[ROWS_STAT_NAME] = int(values[14])
    return out

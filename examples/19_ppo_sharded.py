"""Example 18's loop on an env that is cut over devices: `make_vec(..., devices=[...])` builds one vector env per device on a slice of
the lanes (the same seed, the slice's first lane as lane_offset: together they ARE the one big env, bit for bit), `Replicas` keeps
a copy of the networks on every device, `env.collect` runs every shard's closed loop with its own copy and merges the running
normalisers of all shards, and `ppo_grad_sharded` makes ONE gradient of the shards' minibatches: the advantages are normalised and
the rows weighted over the valid rows of all shards, the shards' raw sums are added before the finish formulas run. One process,
one engine and one stream per device, no collective; what crosses devices are torch copies of a few doubles and one flat gradient
per shard, and nothing waits for the host.

A minibatch is one index list per shard: every shard draws its own permutation of its own rows, and minibatch i of the joint batch
is the i-th piece of each. The optimiser steps the master parameters on devices[0]; `rep.sync()` hands them to the copies.

    python examples/19_ppo_sharded.py [num_envs] [iterations] [device ...]      (default devices: cuda:0 twice)
"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pyflyt_amd import Adam, MLPPolicy, Replicas, minibatches, mlp, ppo_grad_sharded, ppo_stats_dict
from pyflyt_amd.gym_envs import make_vec

num_envs = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
iterations = int(sys.argv[2]) if len(sys.argv) > 2 else 10
devices = sys.argv[3:] or ["cuda:0"] * 2
K, EPOCHS, MINIBATCHES, CLIP, LR = 64, 4, 4, 0.2, 3e-4
CLIP_VF, BOUNDS_COEF, TARGET_KL = 0.2, 1e-4, 0.01

env = make_vec("PyFlyt/QuadX-Hover-v4", num_envs=num_envs, devices=devices, seed=0, max_duration_seconds=1.0)  # (40 steps: episodes finish inside a batch)
obs, _ = env.reset(seed=0)
G, dev, D = len(env.shards), env.devices[0], obs[0].shape[1]
torch.manual_seed(0)
nn = torch.nn
actor = nn.Sequential(nn.Linear(D, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4)).to(dev)
critic = nn.Sequential(nn.Linear(D, 64), nn.Tanh(), nn.Linear(64, 1)).to(dev)
log_std = nn.Parameter(torch.full((4,), -0.5, device=dev))
rep = Replicas(dict(actor=actor, critic=critic, log_std=log_std), env.devices)  # rep[0]: the masters themselves
policies = [MLPPolicy.from_torch(rep[g]["actor"], log_std=rep[g]["log_std"]) for g in range(G)]  # each refers to its device's copy
params = list(actor.parameters()) + list(critic.parameters()) + [log_std]
lr_tensor = torch.full((1,), LR, device=dev)
opt = Adam(env.shards[0], params, lr=lr_tensor, max_grad_norm=0.5, target_kl=TARGET_KL, kl_stop=1.5, kl_lr=dict(factor=1.5, low=0.5, high=2.0, min=1e-6, max=1e-2))
bounds = (env.single_action_space.low, env.single_action_space.high)
shuffles = [torch.Generator(device=d).manual_seed(g) for g, d in enumerate(env.devices)]


def set_obs_stats():
    """The global normaliser's statistics, folded into every shard's policy; returns them per device for the critic and the epochs."""
    mean, std = env.obs_rms.mean, env.obs_rms.std()  # (on devices[0]; empty moments: mean 0, std 1)
    stats = [(mean.to(d), std.to(d)) for d in env.devices]
    for p, (mu, sd) in zip(policies, stats):
        p.set_obs_stats(mu, sd)
    return stats


norm = set_obs_stats()
for it in range(iterations):
    critics = [lambda o, g=g: mlp(env.shards[g], (o - norm[g][0]) / norm[g][1], rep[g]["critic"]) for g in range(G)]
    with torch.no_grad():
        batches = env.collect(policies, critics, K, gamma=0.99, lam=0.95, stats=True, normalize_reward=True)
    xs = [(b["obs"].reshape(-1, D) - mu) / sd for b, (mu, sd) in zip(batches, norm)]
    for epoch in range(EPOCHS):
        pieces = [minibatches(x.shape[0], MINIBATCHES, device=x.device, generator=gen) for x, gen in zip(xs, shuffles)]
        for i in range(MINIBATCHES):
            opt.zero_grad(set_to_none=True)
            stats = ppo_grad_sharded(env, xs, rep, batches, rows=[p[i] for p in pieces], clip=CLIP, vf_coef=1.0, ent_coef=0.0, normalize_advantage=True,
                                     clip_vf=CLIP_VF, action_bounds=bounds, bounds_coef=BOUNDS_COEF)
            opt.step(stats=stats, adapt_lr=epoch == EPOCHS - 1 and i == MINIBATCHES - 1)
            rep.sync()
    norm = set_obs_stats()
    s, p, a, k = env.episode_summary_dict(), ppo_stats_dict(stats, options=True, rows=True), opt.stats_dict(), opt.kl_dict()  # (the host synchronisations)
    print(f"iter {it}: {G} shards, {s['episodes']} episodes, mean return {s['return_mean']:.4f}, loss {p['loss']:.4f}, kl {k['approx_kl']:.3e}, "
          f"minibatch rows {p['valid_rows']} valid, out of range {p['index_out_of_range']}, vclip fraction {p['value_clip_fraction']:.4f}, "
          f"gated steps {k['gated_steps']} of {(it + 1) * EPOCHS * MINIBATCHES}, lr {k['lr']:.3e}, steps {a['step']}")

env.close()

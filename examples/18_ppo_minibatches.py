"""Example 16's loop with shuffled minibatches: every epoch draws one permutation of the batch's rows on the device
(`minibatches`), and every minibatch is one `ppo_grad(..., rows=idx)` and one optimiser step. No row is gathered or copied:
the kernels of `ppo_grad` read their rows through the index list, and give the bits they would give on gathered copies. The
advantages are normalised per minibatch, as the common PPO implementations do; invalid rows stay where they are and are dropped by
selection, so a minibatch's weight 1 / c is taken over its own valid rows. An epoch is still nothing but this library's launches
and one `torch.randperm`, and nothing in it waits for the host.

With the KL control of example 16, a step that pushes the measured KL over `kl_stop * target_kl` closes the gate for the next
minibatch's step; that minibatch measures the KL of its own rows and opens it again if they are under the limit. The learning rate
adapts on the last minibatch of a batch only.

    python examples/18_ppo_minibatches.py [num_envs] [iterations]
"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pyflyt_amd import Adam, MLPPolicy, minibatches, mlp, ppo_grad, ppo_stats_dict
from pyflyt_amd.gym_envs import make_vec

num_envs = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
iterations = int(sys.argv[2]) if len(sys.argv) > 2 else 10
K, EPOCHS, MINIBATCHES, CLIP, LR = 64, 4, 4, 0.2, 3e-4
CLIP_VF, BOUNDS_COEF, TARGET_KL = 0.2, 1e-4, 0.01

env = make_vec("PyFlyt/QuadX-Hover-v4", num_envs=num_envs, seed=0, max_duration_seconds=1.0)  # (40 steps: episodes finish inside a batch)
obs, _ = env.reset(seed=0)
dev, D = obs.device, obs.shape[1]
torch.manual_seed(0)
nn = torch.nn
actor = nn.Sequential(nn.Linear(D, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4)).to(dev)
critic = nn.Sequential(nn.Linear(D, 64), nn.Tanh(), nn.Linear(64, 1)).to(dev)
log_std = nn.Parameter(torch.full((4,), -0.5, device=dev))
policy = MLPPolicy.from_torch(actor, log_std=log_std)  # refers to the parameters' storage
policy.set_obs_stats(env.obs_rms.mean, env.obs_rms.std())  # (empty moments: mean 0, std 1)
params = list(actor.parameters()) + list(critic.parameters()) + [log_std]
lr_tensor = torch.full((1,), LR, device=dev)  # read by the optimiser's kernel and rewritten by the control's
opt = Adam(env, params, lr=lr_tensor, max_grad_norm=0.5, target_kl=TARGET_KL, kl_stop=1.5, kl_lr=dict(factor=1.5, low=0.5, high=2.0, min=1e-6, max=1e-2))
bounds = (env.single_action_space.low, env.single_action_space.high)
M = K * num_envs  # the rows of a batch
shuffle = torch.Generator(device=dev).manual_seed(0)

for it in range(iterations):
    mu, sd = policy.obs_mean.clone(), policy.obs_std.clone()  # the statistics this batch is collected (and learned from) with
    with torch.no_grad():  # (the critic of the rollout: the same call, no graph)
        b = env.collect(policy, lambda o: mlp(env, (o - mu) / sd, critic), K, gamma=0.99, lam=0.95, stats=True, normalize_reward=True)
    o = (b["obs"].reshape(-1, D) - mu) / sd  # (the normalisation stays an element-wise pre-pass over the whole batch, once)
    for epoch in range(EPOCHS):
        for i, idx in enumerate(minibatches(M, MINIBATCHES, device=dev, generator=shuffle)):  # (one permutation per epoch; idx: int32 [M / 4])
            opt.zero_grad(set_to_none=True)
            stats = ppo_grad(env, o, actor, critic, log_std, b, clip=CLIP, vf_coef=1.0, ent_coef=0.0, normalize_advantage=True, clip_vf=CLIP_VF,
                             action_bounds=bounds, bounds_coef=BOUNDS_COEF, rows=idx)  # (the rows idx names, read where they lie)
            opt.step(stats=stats, adapt_lr=epoch == EPOCHS - 1 and i == MINIBATCHES - 1)
    policy.set_obs_stats(env.obs_rms.mean, env.obs_rms.std())  # fold the updated statistics (and the stepped first layer) for the next rollout
    s, p, a, k = env.episode_summary_dict(), ppo_stats_dict(stats, options=True, rows=True), opt.stats_dict(), opt.kl_dict()  # (the host synchronisations)
    print(f"iter {it}: {s['episodes']} episodes, mean return {s['return_mean']:.4f}, loss {p['loss']:.4f}, kl {k['approx_kl']:.3e}, "
          f"minibatch rows {p['valid_rows']} valid of {idx.numel()}, out of range {p['index_out_of_range']}, vclip fraction {p['value_clip_fraction']:.4f}, "
          f"gated steps {k['gated_steps']} of {(it + 1) * EPOCHS * MINIBATCHES}, lr {k['lr']:.3e}, steps {a['step']}")

env.close()

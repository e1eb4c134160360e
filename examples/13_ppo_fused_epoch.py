"""Example 11 with the epoch in one call: `ppo_grad` (pf_ppo_grad) leaves in .grad what the two `mlp` forwards, `ppo_loss` and
`backward()` left there -- the network gradients bit for bit -- without the mean, value and per-row gradient tensors between them: the
tile kernel of the backward computes the output layer and the loss's per-row gradients where it used to load them. An epoch is
`opt.zero_grad(); stats = ppo_grad(...); opt.step()`: seven launches and the optimiser's two, and nothing in it waits for the host.

    python examples/13_ppo_fused_epoch.py [num_envs] [iterations]
"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pyflyt_amd import Adam, MLPPolicy, mlp, ppo_grad, ppo_stats_dict
from pyflyt_amd.gym_envs import make_vec

num_envs = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
iterations = int(sys.argv[2]) if len(sys.argv) > 2 else 10
K, EPOCHS, CLIP, LR = 64, 4, 0.2, 3e-4

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
lr_tensor = torch.full((), LR, device=dev)  # read by the kernel at every step
opt = Adam(env, params, lr=lr_tensor, max_grad_norm=0.5)

for it in range(iterations):
    lr_tensor.fill_(LR * (1.0 - it / iterations))  # the linear anneal: a device-side write, no synchronisation
    mu, sd = policy.obs_mean.clone(), policy.obs_std.clone()  # the statistics this batch is collected (and learned from) with
    with torch.no_grad():  # (the critic of the rollout: the same call, no graph)
        b = env.collect(policy, lambda o: mlp(env, (o - mu) / sd, critic), K, gamma=0.99, lam=0.95, stats=True, normalize_reward=True)
    o = (b["obs"].reshape(-1, D) - mu) / sd  # (the normalisation stays an element-wise pre-pass)
    for _ in range(EPOCHS):  # (full batch: minibatching is the learner's business)
        opt.zero_grad(set_to_none=True)
        stats = ppo_grad(env, o, actor, critic, log_std, b, clip=CLIP, vf_coef=1.0, ent_coef=0.0, normalize_advantage=True)
        opt.step()
    policy.set_obs_stats(env.obs_rms.mean, env.obs_rms.std())  # fold the updated statistics (and the stepped first layer) for the next rollout
    s, p, a = env.episode_summary_dict(), ppo_stats_dict(stats), opt.stats_dict()  # (the three host synchronisations of the iteration)
    print(f"iteration {it}: {s['episodes']} episodes finished, mean episode return {s['return_mean']:.4f}, mean episode length {s['length_mean']:.2f}, "
          f"loss {p['loss']:.4f}, approx_kl {p['approx_kl']:.3e}, clip_fraction {p['clip_fraction']:.4f}, explained variance {p['explained_variance']:.4f}, "
          f"lr {a['lr']:.3e}, grad_norm {a['grad_norm']:.4f}, clip_coef {a['clip_coef']:.4f}")

env.close()

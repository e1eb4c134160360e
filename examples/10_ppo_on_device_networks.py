"""Example 08 with both networks evaluated and differentiated by `pyflyt_amd.mlp` instead of torch modules: an epoch is two
`mlp` forwards (pf_mlp_forward, the rollout policy's own kernel), one `ppo_loss`, one `backward()` (pf_mlp_backward: the hidden
activations are computed again from the observations, none is ever written to memory) and the optimiser's step -- the only torch
work left. The modules stay what they are: torch.nn.Sequential, their parameters updated in place by torch.optim.

What that buys is memory: torch keeps every [rows, 64] activation of both networks until the backward (5.4 GB at 65 536
envs x 64 steps, measured); this path keeps none. And time: at that size an epoch's network work takes 7.4 ms against 26.0 ms
through the modules on one MI355X (tools/bench_mlp.py measures it on your device and at your size).

    python examples/10_ppo_on_device_networks.py [num_envs] [iterations]
"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pyflyt_amd import MLPPolicy, mlp, ppo_loss, ppo_stats_dict
from pyflyt_amd.gym_envs import make_vec

num_envs = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
iterations = int(sys.argv[2]) if len(sys.argv) > 2 else 10
K, EPOCHS, CLIP = 64, 4, 0.2

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
opt = torch.optim.Adam(params, lr=3e-4)

for it in range(iterations):
    mu, sd = policy.obs_mean.clone(), policy.obs_std.clone()  # the statistics this batch is collected (and learned from) with
    with torch.no_grad():  # (the critic of the rollout: the same call, no graph)
        b = env.collect(policy, lambda o: mlp(env, (o - mu) / sd, critic), K, gamma=0.99, lam=0.95, stats=True, normalize_reward=True)
    o = (b["obs"].reshape(-1, D) - mu) / sd  # (the normalisation stays an element-wise pre-pass; o is not modified before backward())
    for _ in range(EPOCHS):  # (full batch: minibatching is the learner's business)
        loss, stats = ppo_loss(env, mlp(env, o, actor), log_std, mlp(env, o, critic), b, clip=CLIP, vf_coef=1.0, ent_coef=0.0, normalize_advantage=True)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    policy.set_obs_stats(env.obs_rms.mean, env.obs_rms.std())  # fold the updated statistics (and the stepped first layer) for the next rollout
    s, p = env.episode_summary_dict(), ppo_stats_dict(stats)  # (the two host synchronisations of the iteration)
    print(f"iteration {it}: {s['episodes']} episodes finished, mean episode return {s['return_mean']:.4f}, mean episode length {s['length_mean']:.2f}, "
          f"loss {p['loss']:.4f}, approx_kl {p['approx_kl']:.3e}, clip_fraction {p['clip_fraction']:.4f}, explained variance {p['explained_variance']:.4f}")

env.close()

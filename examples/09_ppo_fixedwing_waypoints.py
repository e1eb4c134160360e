"""Example 08's loop on PyFlyt/Fixedwing-Waypoints-v4. The library has no fused rollout launch for the aircraft, so `env.collect`
takes the stepwise closed loop: per step one `pf_policy_act` launch (the policy MLP over all envs on the matrix cores) and one
`pf_env_step`, both writing straight into the batch's trajectory rows -- the same call and the same batch dict as on the quadrotor.

    python examples/09_ppo_fixedwing_waypoints.py [num_envs] [iterations]
"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pyflyt_amd import MLPPolicy, ppo_loss, ppo_stats_dict
from pyflyt_amd.gym_envs import make_vec

num_envs = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
iterations = int(sys.argv[2]) if len(sys.argv) > 2 else 10
K, EPOCHS, CLIP = 64, 4, 0.2

env = make_vec("PyFlyt/Fixedwing-Waypoints-v4", num_envs=num_envs, seed=0, max_duration_seconds=2.0)  # (60 steps: episodes finish inside a batch)
env.reset(seed=0)
dev, D = env.device, env.engine.obs_dim  # (the policy reads the engine's flat rows: attitude, then the target deltas)
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
    b = env.collect(policy, lambda o: critic((o - mu) / sd), K, gamma=0.99, lam=0.95, stats=True, normalize_reward=True)  # fused=None: stepwise here
    o = (b["obs"].reshape(-1, D) - mu) / sd
    for _ in range(EPOCHS):  # (full batch: minibatching is the learner's business)
        loss, stats = ppo_loss(env, actor(o), log_std, critic(o), b, clip=CLIP, vf_coef=1.0, ent_coef=0.0, normalize_advantage=True)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    policy.set_obs_stats(env.obs_rms.mean, env.obs_rms.std())  # fold the updated statistics (and the stepped first layer) for the next rollout
    s, p = env.episode_summary_dict(), ppo_stats_dict(stats)  # (the two host synchronisations of the iteration)
    print(f"iteration {it} (stepwise collect): {s['episodes']} episodes finished, mean episode return {s['return_mean']:.4f}, "
          f"mean episode length {s['length_mean']:.2f}, loss {p['loss']:.4f}, approx_kl {p['approx_kl']:.3e}, "
          f"clip_fraction {p['clip_fraction']:.4f}, explained variance {p['explained_variance']:.4f}")

env.close()

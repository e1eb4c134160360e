"""Example 06 with what a gymnasium user wraps around the env before training: episode statistics (RecordEpisodeStatistics) and
observation / reward normalisation (NormalizeObservation, NormalizeReward). `env.collect(..., stats=True, normalize_reward=True)`
runs pf_traj_stats on the rollout's trajectory: it returns every finished episode's return and length, keeps the running moments
behind `env.obs_rms` / `env.ret_rms` on the device, and hands pf_gae the reward divided by the running standard deviation of the
discounted return. The observation statistics go into the policy's first layer (`policy.set_obs_stats`), so the rollout kernel
normalises for free; the learner applies the same statistics to its inputs.

    python examples/07_ppo_hover_normalized.py [num_envs] [iterations]
"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pyflyt_amd import MLPPolicy
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
    b = env.collect(policy, lambda o: critic((o - mu) / sd), K, gamma=0.99, lam=0.95, stats=True, normalize_reward=True)
    valid = b["valid"].reshape(-1)
    w = valid.float() / valid.sum()  # the mean over the real transitions
    o, a = (b["obs"].reshape(-1, D) - mu) / sd, b["actions"].reshape(-1, 4)
    logp_old, ret = b["logp"].reshape(-1), b["returns"].reshape(-1)
    adv = b["advantages"].reshape(-1)
    adv = adv - (adv * w).sum()
    adv = adv / (adv.pow(2) * w).sum().sqrt().clamp_min(1e-8)
    for _ in range(EPOCHS):  # (full batch: minibatching is the learner's business)
        logp = torch.distributions.Normal(actor(o), log_std.exp()).log_prob(a).sum(-1)
        ratio = (logp - logp_old).exp()
        surrogate = torch.minimum(ratio * adv, ratio.clamp(1 - CLIP, 1 + CLIP) * adv)
        loss = -(surrogate * w).sum() + 0.5 * ((critic(o).squeeze(-1) - ret).pow(2) * w).sum()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    policy.set_obs_stats(env.obs_rms.mean, env.obs_rms.std())  # fold the updated statistics (and the stepped first layer) for the next rollout
    s = env.episode_summary_dict()  # (the one host synchronisation of the iteration)
    print(f"iteration {it}: {s['episodes']} episodes finished, mean episode return {s['return_mean']:.4f}, mean episode length {s['length_mean']:.2f}, "
          f"return std of the reward scale {float(env.ret_rms.std()):.4f}, loss {loss.item():.4f}")

env.close()

"""Example 12's self-play loop with what examples 07-13 wrap around the vector envs: episode statistics and observation / reward
normalisation. `env.collect(..., opponent=..., normalize_reward=True)` runs pf_traj_stats_masked on the batch with `valid` as its
mask: the steps a finished aircraft sits out, the step that resets its copy and the opponent's lanes are in no return, no length and
no moment. It keeps the running moments behind `env.obs_rms` / `env.ret_rms` on the device and hands pf_gae the reward divided by the
running standard deviation of the discounted return. The observation statistics go into the policy's first layer
(`policy.set_obs_stats`); the learner applies the same statistics to its inputs. The frozen opponent keeps the statistics it was
frozen with, refreshed together with its weights.

With self-play the loss says little about progress; the loop prints what `env.episode_summary_dict()` holds of the episodes team 0
finished in the batch: how many, their mean return and length, and how they ended.

    python examples/14_ppo_dogfight_selfplay_stats.py [num_envs] [iterations]
"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import copy
import torch
from pyflyt_amd import Adam, MLPPolicy, mlp, ppo_loss, ppo_stats_dict
from pyflyt_amd.pz_envs import MAFixedwingDogfightEnv

num_envs = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
iterations = int(sys.argv[2]) if len(sys.argv) > 2 else 10
K, EPOCHS, CLIP, LR, REFRESH = 64, 4, 0.2, 3e-4, 3

env = MAFixedwingDogfightEnv(team_size=2, num_envs=num_envs, seed=0, max_duration_seconds=1.5)  # (45 steps: episodes finish inside a batch)
env.reset(seed=0)
dev, D = env.engine.device, env.engine.obs_dim
torch.manual_seed(0)
nn = torch.nn
actor = nn.Sequential(nn.Linear(D, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4)).to(dev)
critic = nn.Sequential(nn.Linear(D, 64), nn.Tanh(), nn.Linear(64, 1)).to(dev)
log_std = nn.Parameter(torch.full((4,), -0.5, device=dev))
policy = MLPPolicy.from_torch(actor, log_std=log_std)  # refers to the parameters' storage
policy.set_obs_stats(env.obs_rms.mean, env.obs_rms.std())  # (empty moments: mean 0, std 1)
frozen_actor, frozen_log_std = copy.deepcopy(actor), log_std.detach().clone()
opponent = MLPPolicy.from_torch(frozen_actor, log_std=frozen_log_std)  # refers to the copies': stays as it is until the next refresh
opponent.set_obs_stats(policy.obs_mean, policy.obs_std)  # (copied: the opponent's own, frozen with its weights)
params = list(actor.parameters()) + list(critic.parameters()) + [log_std]
opt = Adam(env, params, lr=LR, max_grad_norm=0.5)

for it in range(iterations):
    if it and it % REFRESH == 0:  # the opponent catches up, weights and statistics: in place, then folded again
        with torch.no_grad():
            for p, q in zip(frozen_actor.parameters(), actor.parameters()):
                p.copy_(q)
            frozen_log_std.copy_(log_std)
        opponent.set_obs_stats(policy.obs_mean, policy.obs_std)
    mu, sd = policy.obs_mean.clone(), policy.obs_std.clone()  # the statistics this batch is collected (and learned from) with
    with torch.no_grad():
        b = env.collect(policy, lambda o: mlp(env, (o - mu) / sd, critic), K, gamma=0.99, lam=0.95, opponent=opponent, normalize_reward=True)
    o = (b["obs"].reshape(-1, D) - mu) / sd
    for _ in range(EPOCHS):  # (full batch: minibatching is the learner's business)
        loss, stats = ppo_loss(env, mlp(env, o, actor), log_std, mlp(env, o, critic), b, clip=CLIP, vf_coef=1.0, ent_coef=0.0, normalize_advantage=True)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    policy.set_obs_stats(env.obs_rms.mean, env.obs_rms.std())  # fold the updated statistics (and the stepped first layer) for the next rollout
    s, p = env.episode_summary_dict(), ppo_stats_dict(stats)  # (the two host synchronisations of the iteration)
    print(f"iteration {it}: {s['episodes']} episodes finished, mean episode return {s['return_mean']:.4f}, mean episode length {s['length_mean']:.2f}, "
          f"{s['terminated']} terminated / {s['truncated']} truncated, return std of the reward scale {float(env.ret_rms.std()):.4f}, "
          f"loss {p['loss']:.4f}, approx_kl {p['approx_kl']:.3e}")

env.close()

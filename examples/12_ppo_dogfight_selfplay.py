"""Example 11's loop on the team dogfight: PPO by self-play, nothing but this library's kernels between the observation and the
optimiser's step. `env.collect` runs the closed loop on the device (pf_policy_act, pf_env_step, pf_world_sync, pf_env_reset per
step): a copy of the env whose four aircraft have all finished is reset between two steps, and `valid` marks the steps that were real
transitions. Team 0 flies the actor that is being trained; team 1 flies a frozen copy of it, refreshed every few iterations, from
the same observations -- its lanes are never valid, so the batch holds team 0's experience only.

The batch is flat, [k, num_envs * 4, ...] with lane = copy * 4 + aircraft: `.view(k, num_envs, 4, ...)` reads it per copy. Episode
statistics (collect's stats= on the vector envs) do not exist for the multi-agent batch; the loop prints the mean reward per valid
step and the share of valid steps instead.

    python examples/12_ppo_dogfight_selfplay.py [num_envs] [iterations]
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
frozen_actor, frozen_log_std = copy.deepcopy(actor), log_std.detach().clone()
opponent = MLPPolicy.from_torch(frozen_actor, log_std=frozen_log_std)  # refers to the copies': stays as it is until the next refresh
params = list(actor.parameters()) + list(critic.parameters()) + [log_std]
opt = Adam(env, params, lr=LR, max_grad_norm=0.5)

for it in range(iterations):
    if it and it % REFRESH == 0:  # the opponent catches up: in place, so the policy block's pointers stay good
        with torch.no_grad():
            for p, q in zip(frozen_actor.parameters(), actor.parameters()):
                p.copy_(q)
            frozen_log_std.copy_(log_std)
    with torch.no_grad():
        b = env.collect(policy, lambda o: mlp(env, o, critic), K, gamma=0.99, lam=0.95, opponent=opponent)
    o = b["obs"].reshape(-1, D)
    for _ in range(EPOCHS):  # (full batch: minibatching is the learner's business)
        loss, stats = ppo_loss(env, mlp(env, o, actor), log_std, mlp(env, o, critic), b, clip=CLIP, vf_coef=1.0, ent_coef=0.0, normalize_advantage=True)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    valid = b["valid"]
    share = valid.float().mean()
    reward = torch.where(valid, b["reward"], torch.zeros_like(b["reward"])).sum() / valid.sum().clamp(min=1)
    p = ppo_stats_dict(stats)  # (the host synchronisation of the iteration)
    print(f"iteration {it}: reward per valid step {float(reward):.4f}, valid share {float(share):.4f}, loss {p['loss']:.4f}, "
          f"approx_kl {p['approx_kl']:.3e}, clip_fraction {p['clip_fraction']:.4f}, explained variance {p['explained_variance']:.4f}")

env.close()

"""A complete, minimal PPO loop on QuadX-Hover. `env.collect(policy, value_fn, k)` is the whole data side: the closed-loop rollout with
the policy MLP on the device, the critic through torch, then pf_gae for the validity mask, advantages, returns and log-probabilities.
The learner below is plain torch: a clipped surrogate masked by `valid`, a value loss on `returns`, Adam stepping the parameters IN
PLACE -- the policy refers to the same tensors, so the next collect() rolls out the updated network.

    python examples/06_ppo_hover.py [num_envs] [iterations]
"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pyflyt_amd import MLPPolicy
from pyflyt_amd.gym_envs import make_vec

num_envs = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
iterations = int(sys.argv[2]) if len(sys.argv) > 2 else 10
K, EPOCHS, CLIP = 64, 4, 0.2

env = make_vec("PyFlyt/QuadX-Hover-v4", num_envs=num_envs, seed=0)  # NEXT_STEP auto-reset: some steps only reset a lane (valid = False)
obs, _ = env.reset(seed=0)
dev, D = obs.device, obs.shape[1]
torch.manual_seed(0)
nn = torch.nn
actor = nn.Sequential(nn.Linear(D, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4)).to(dev)
critic = nn.Sequential(nn.Linear(D, 64), nn.Tanh(), nn.Linear(64, 1)).to(dev)
log_std = nn.Parameter(torch.full((4,), -0.5, device=dev))
policy = MLPPolicy.from_torch(actor, log_std=log_std)  # refers to the parameters' storage
params = list(actor.parameters()) + list(critic.parameters()) + [log_std]
before = torch.cat([p.detach().reshape(-1).clone() for p in params])
opt = torch.optim.Adam(params, lr=3e-4)

for it in range(iterations):
    b = env.collect(policy, critic, K, gamma=0.99, lam=0.95)
    valid = b["valid"].reshape(-1)
    w = valid.float() / valid.sum()  # the mean over the real transitions
    o, a = b["obs"].reshape(-1, D), b["actions"].reshape(-1, 4)
    logp_old, ret = b["logp"].reshape(-1), b["returns"].reshape(-1)
    adv = b["advantages"].reshape(-1)
    adv = (adv - (adv * w).sum()) / ((adv - (adv * w).sum()).pow(2) * w).sum().sqrt().clamp_min(1e-8)
    mean_reward = (b["reward"].reshape(-1) * w).sum()
    for _ in range(EPOCHS):  # (full batch: minibatching is the learner's business)
        logp = torch.distributions.Normal(actor(o), log_std.exp()).log_prob(a).sum(-1)
        ratio = (logp - logp_old).exp()
        surrogate = torch.minimum(ratio * adv, ratio.clamp(1 - CLIP, 1 + CLIP) * adv)
        loss = -(surrogate * w).sum() + 0.5 * ((critic(o).squeeze(-1) - ret).pow(2) * w).sum()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    print(f"iteration {it}: mean reward per valid step {mean_reward.item():.4f}, {int(valid.sum())} of {valid.numel()} steps valid, "
          f"{int((b['terminated'] | b['truncated']).sum())} episodes ended, loss {loss.item():.4f}")

after = torch.cat([p.detach().reshape(-1) for p in params])
print(f"parameters moved by {(after - before).abs().max().item():.3e}")
env.close()

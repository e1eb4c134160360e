"""Four checkpoints of a policy flown side by side in ONE batch of QuadX-Hover, and how the episodes of each ended. `env.rollout` takes a
list of policies: the envs are cut into contiguous, near-equal segments (or `group=` says which policy flies which env), one
pf_policy_pool_plan sorts the envs by policy, and every step is one pf_policy_act_pool -- each env evaluated once, by its own policy,
with the bits that policy alone would give it -- and one pf_env_step. `outcomes=True` adds pf_episode_outcomes to every step:
`outcome_counts` [4, 16] holds one row per policy, and `env.episode_outcomes_dict()` reads it back by name, the one host
synchronisation of the tournament.

The "checkpoints" here are one random network with its output layer scaled by 0, 0.5, 1 and 2: the first commands nothing but noise,
the last the most. A real tournament loads four saved state dicts instead.

    python examples/17_checkpoint_tournament.py [num_envs] [steps]
"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import copy
import torch
from pyflyt_amd import MLPPolicy
from pyflyt_amd.gym_envs import make_vec

num_envs = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
GAINS = (0.0, 0.5, 1.0, 2.0)

env = make_vec("PyFlyt/QuadX-Hover-v4", num_envs=num_envs, seed=0, max_duration_seconds=1.0, flight_dome_size=1.5)  # (40 steps, a small dome)
obs, _ = env.reset(seed=0)
dev, D = obs.device, obs.shape[1]
torch.manual_seed(0)
nn = torch.nn
base = nn.Sequential(nn.Linear(D, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4)).to(dev)
checkpoints = []
for gain in GAINS:
    net = copy.deepcopy(base)
    with torch.no_grad():
        net[-1].weight.mul_(gain)
        net[-1].bias.mul_(gain)
    checkpoints.append(MLPPolicy.from_torch(net, log_std=torch.full((4,), -1.0, device=dev)))

out = env.rollout(checkpoints, steps, outcomes=True)  # (obs, reward, terminated, truncated, actions, outcome, outcome_counts, infos)
reward, counts = out[1], out[6]
rows = env.episode_outcomes_dict(counts)  # (the host synchronisation)
per_policy = reward.view(steps, len(GAINS), -1).mean(dim=(0, 2)).tolist() if num_envs % len(GAINS) == 0 else [float("nan")] * len(GAINS)
for p, (gain, r, mean_reward) in enumerate(zip(GAINS, rows, per_policy)):
    print(f"policy {p} (output gain {gain}): {r['episodes']} episodes, {r['truncated']} reached the time limit, {r['collision']} collision, "
          f"{r['out_of_bounds']} out of bounds, {r['nonfinite']} nonfinite; mean reward per step {mean_reward:.4f}")

env.close()

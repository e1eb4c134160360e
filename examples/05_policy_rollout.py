"""A closed-loop rollout in one launch: a small MLP policy evaluated on the device, per env, between two env steps
(`env.rollout(policy, k)` -> pf_rollout_policy). The policy refers to the torch parameters: train them in place and roll out again."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pyflyt_amd import MLPPolicy
from pyflyt_amd.gym_envs import make_vec

num_envs = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
env = make_vec("PyFlyt/QuadX-Hover-v4", num_envs=num_envs, seed=0)
obs, info = env.reset(seed=0)
torch.manual_seed(0)
net = torch.nn.Sequential(torch.nn.Linear(obs.shape[1], 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(),
                          torch.nn.Linear(64, 4)).to(obs.device)
policy = MLPPolicy.from_torch(net, log_std=torch.full((4,), -1.0, device=obs.device))
episodes, ret = 0, 0.0
for _ in range(2):  # 2 x 50 steps; the second call acts on the last observation of the first
    obs, reward, terminated, truncated, actions, info = env.rollout(policy, 50)
    episodes += int((terminated | truncated).sum())
    ret += float(reward.sum(0).mean())
print(f"{num_envs} envs x 100 policy steps in 2 launches: {episodes} episodes ended, mean return {ret:.2f}, "
      f"collisions {int(info['collision'].sum())}, out of bounds {int(info['out_of_bounds'].sum())}")
env.close()

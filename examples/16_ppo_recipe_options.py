"""Example 13's loop with PPO's usual options, all of them on the device: a clipped value loss (`clip_vf`), a penalty on means that
leave the env's action box (`action_bounds`, `bounds_coef`), and the KL decisions -- skip the optimiser's step once the measured KL is
over the limit, adapt the learning rate to it -- taken by `pf_kl_control` in front of a gated Adam step. An epoch is still
`opt.zero_grad(); stats = ppo_grad(...); opt.step(stats=stats)`: seven launches, the control's one and the optimiser's two, and
nothing in it waits for the host. Once a step has pushed the KL over `kl_stop * target_kl` the later epochs on the same batch see
unchanged parameters, measure the same KL and are skipped too: early stopping without a host read. The learning rate adapts on the
last epoch of a batch only (`adapt_lr=False` in the others).

Where the defaults come from: clip_vf = 0.2 is the value-clipping range of the common PPO implementations (the same number as the
policy's clip); bounds_coef = 1e-4 and the adaptive-KL schedule (lr / 1.5 above 2 x target_kl, lr x 1.5 below 0.5 x target_kl, within
[1e-6, 1e-2]) follow the recipe widely used for PPO on tens of thousands of parallel simulated envs; target_kl = 0.01 with a stop at
1.5 x is Stable-Baselines3's early stop. Nobody has tuned them for these envs.

    python examples/16_ppo_recipe_options.py [num_envs] [iterations]
"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pyflyt_amd import Adam, MLPPolicy, mlp, ppo_grad, ppo_stats_dict
from pyflyt_amd.gym_envs import make_vec

num_envs = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
iterations = int(sys.argv[2]) if len(sys.argv) > 2 else 10
K, EPOCHS, CLIP, LR = 64, 4, 0.2, 3e-4
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

for it in range(iterations):
    mu, sd = policy.obs_mean.clone(), policy.obs_std.clone()  # the statistics this batch is collected (and learned from) with
    with torch.no_grad():  # (the critic of the rollout: the same call, no graph)
        b = env.collect(policy, lambda o: mlp(env, (o - mu) / sd, critic), K, gamma=0.99, lam=0.95, stats=True, normalize_reward=True)
    o = (b["obs"].reshape(-1, D) - mu) / sd  # (the normalisation stays an element-wise pre-pass)
    for epoch in range(EPOCHS):  # (full batch: minibatching is the learner's business)
        opt.zero_grad(set_to_none=True)
        stats = ppo_grad(env, o, actor, critic, log_std, b, clip=CLIP, vf_coef=1.0, ent_coef=0.0, normalize_advantage=True, clip_vf=CLIP_VF,
                         action_bounds=bounds, bounds_coef=BOUNDS_COEF)  # (values_old: the batch's values)
        opt.step(stats=stats, adapt_lr=epoch == EPOCHS - 1)
    policy.set_obs_stats(env.obs_rms.mean, env.obs_rms.std())  # fold the updated statistics (and the stepped first layer) for the next rollout
    s, p, a, k = env.episode_summary_dict(), ppo_stats_dict(stats, options=True), opt.stats_dict(), opt.kl_dict()  # (the host synchronisations of the iteration)
    print(f"iter {it}: {s['episodes']} episodes, mean return {s['return_mean']:.4f}, loss {p['loss']:.4f}, kl {k['approx_kl']:.3e}, "
          f"vclip fraction {p['value_clip_fraction']:.4f}, bounds loss {p['bounds_loss']:.3e}, gated steps {k['gated_steps']} of {(it + 1) * EPOCHS}, "
          f"lr {k['lr']:.3e}, steps {a['step']}")

env.close()

"""Example 14's self-play loop against a small league: team 1 is flown by TWO earlier snapshots of the actor at once, and the loop prints
the win rate against each. `env.collect(..., opponent=[older, newer], outcomes=True, pooled=True)` cuts the copies into two contiguous
segments, flies segment p's team 1 with snapshot p (the actor and both snapshots in ONE pf_policy_act_pool per step, every lane evaluated
once by the policy that flies it; without pooled=True, one pf_policy_act over all rows and one merge per snapshot, for the same bits), and adds pf_episode_outcomes to every
step: `outcome_counts` [2, 16] holds, per snapshot, how team 0's episodes ended (collision, out of bounds, team_win, dead, or the time
limit) and how the copies that finished in this batch went -- team 0 wins, team 1 wins, draws. `env.episode_outcomes_dict()` reads the
block back by name: the one host synchronisation the win rate costs.

With a frozen copy of itself as the opponent the mean return says little about progress; the win rate against PAST selves is the
number that should rise. Every REFRESH iterations the older snapshot takes the newer one's place and the newer one the actor's.

    python examples/15_ppo_dogfight_league.py [num_envs] [iterations]
"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import copy
import torch
from pyflyt_amd import Adam, MLPPolicy, mlp, ppo_loss, ppo_stats_dict
from pyflyt_amd.pz_envs import MAFixedwingDogfightEnv

num_envs = int(sys.argv[1]) if len(sys.argv) > 1 else 256
iterations = int(sys.argv[2]) if len(sys.argv) > 2 else 4
K, EPOCHS, CLIP, LR, REFRESH = 64, 4, 0.2, 3e-4, 2

env = MAFixedwingDogfightEnv(team_size=2, num_envs=num_envs, seed=0, max_duration_seconds=1.0)  # (30 steps: copies finish twice inside a batch)
env.reset(seed=0)
dev, D = env.engine.device, env.engine.obs_dim
torch.manual_seed(0)
nn = torch.nn
actor = nn.Sequential(nn.Linear(D, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4)).to(dev)
critic = nn.Sequential(nn.Linear(D, 64), nn.Tanh(), nn.Linear(64, 1)).to(dev)
log_std = nn.Parameter(torch.full((4,), -0.5, device=dev))
policy = MLPPolicy.from_torch(actor, log_std=log_std)  # refers to the parameters' storage
# the league: two snapshots, each a frozen copy of the actor and its log_std that its MLPPolicy refers to
nets = [copy.deepcopy(actor) for _ in range(2)]
stds = [log_std.detach().clone() for _ in range(2)]
league = [MLPPolicy.from_torch(net, log_std=std) for net, std in zip(nets, stds)]
opt = Adam(env, list(actor.parameters()) + list(critic.parameters()) + [log_std], lr=LR, max_grad_norm=0.5)


def overwrite(net, std, src_net, src_std):
    with torch.no_grad():
        for p, q in zip(net.parameters(), src_net.parameters()):
            p.copy_(q)
        std.copy_(src_std)


for it in range(iterations):
    if it and it % REFRESH == 0:  # snapshot 0 (older) <- snapshot 1 (newer) <- the actor: in place, the policies see the new weights
        overwrite(nets[0], stds[0], nets[1], stds[1])
        overwrite(nets[1], stds[1], actor, log_std)
    with torch.no_grad():
        b = env.collect(policy, lambda o: mlp(env, o, critic), K, gamma=0.99, lam=0.95, opponent=league, outcomes=True, pooled=True)
    o = b["obs"].reshape(-1, D)
    for _ in range(EPOCHS):
        loss, stats = ppo_loss(env, mlp(env, o, actor), log_std, mlp(env, o, critic), b, clip=CLIP, vf_coef=1.0, ent_coef=0.0, normalize_advantage=True)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    rows, p = env.episode_outcomes_dict(), ppo_stats_dict(stats)  # (the two host synchronisations of the iteration)
    for name, r in zip(("older", "newer"), rows):
        rate = r["team0_wins"] / r["worlds"] if r["worlds"] else float("nan")
        print(f"iteration {it} vs {name} snapshot: {r['worlds']} copies finished, win rate {rate:.3f} ({r['team0_wins']} won / {r['team1_wins']} lost / "
              f"{r['draws']} drawn); team 0's {r['episodes']} episodes: {r['complete']} team_win, {r['dead']} dead, {r['out_of_bounds']} out of bounds, "
              f"{r['collision']} collision, {r['clean']} time limit, {r['second_word_sum']} hits received")
    print(f"iteration {it}: loss {p['loss']:.4f}, approx_kl {p['approx_kl']:.3e}")

env.close()

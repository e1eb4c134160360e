"""rollout() and collect() of the multi-agent envs (pf_world_sync between the env steps: BatchEngine.rollout_policy_worlds) against the
loop a user writes by hand through the façade -- policy_act, step(dict), a reset of the copies whose agents have all finished --, bit
for bit; the carry over calls; collect()'s batch against a float64 host GAE over each lane's valid runs; the frozen opponent; the
façade after a collect; the self-play example."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pyflyt_amd
from pyflyt_amd import MLPPolicy
from pyflyt_amd.pz_envs import MAFixedwingDogfightEnv, MAQuadXHoverEnv
from test_gpu_gae import gae_bound, logp_bound  # (derived there)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The dogfight: 30-step episodes. Combat arguments widened from test_dogfight_engagements_vs_oracle's (damage 0.006, 45 m, 0.3 rad) until
# aircraft of one copy end at different steps under a random policy: a cone of fire past the beam (the `chasing` half-space binds),
# any range, two hits kill; and a 65 m dome that the outward-flying spawn circle (10-50 m out, 10-50 m up, 20 m/s) crosses at
# scattered steps -- an aircraft out of bounds ends, and its opposite number ends with it by team win. Checked on the fp64 oracle
# (oracle.OracleDogfight on spawns drawn by oracle.dogfight_spawn, normal actions, the same world reset rule) for both team sizes and
# three seeds: 4-10 copies of 16 (7-10 of 11) with agents ending at different steps, 16-28 truncations, valid share 0.64-0.80.
DF_KW = dict(damage_per_hit=0.5, lethal_distance=400.0, lethal_angle_radians=1.6, flight_dome_size=65.0, max_duration_seconds=1.0)
DF_K = 48
# The multi-agent hover: 20-step episodes (the 22nd step truncates), four drones. log_std = 0: unit noise on the body-rate and thrust
# commands. From 1 m up that alone brings down one drone in 64 before the truncation (measured: thrust biases 0 .. 1 end 0-4 episodes
# early); with the thrust head's bias at 1.5 the rate noise tips the drones over under full thrust and about a third of them hit the
# floor, at scattered steps, while the rest fly on to the truncation.
HV_KW = dict(max_duration_seconds=0.5)
HV_E, HV_K, HV_THRUST_BIAS = 16, 40, 1.5


def make_policy(D, W, seed, log_std=0.0, out_bias=None):
    g = torch.Generator().manual_seed(seed)

    def lin(o, i, gain):
        return (torch.randn(o, i, generator=g) * gain / i ** 0.5).to(DEV).contiguous(), torch.zeros(o, device=DEV)

    layers = [lin(32, D, 1.0), lin(32, 32, 1.0), lin(W, 32, 0.3)]
    if out_bias is not None:
        layers[-1][1].copy_(torch.tensor(out_bias))
    return MLPPolicy(layers, "tanh", log_std=None if log_std is None else torch.full((W,), float(log_std), device=DEV))


def make_env(kind, seed=11):
    if kind[0] == "dogfight":
        env = MAFixedwingDogfightEnv(team_size=kind[1], num_envs=kind[2], seed=seed, **DF_KW)
    else:
        env = MAQuadXHoverEnv(num_envs=HV_E, seed=seed, shared_world=kind[1], **HV_KW)
    env.reset(seed=seed)
    return env


def env_policy(env, seed=5):
    hover = isinstance(env, MAQuadXHoverEnv)
    return make_policy(env.engine.obs_dim, env.engine.action_dim, seed, out_bias=[0.0, 0.0, 0.0, HV_THRUST_BIAS] if hover else None)


def reset_copies(env, copies):
    if hasattr(env, "reset_envs"):
        env.reset_envs(copies)
    else:  # (the hover façade has no per-copy reset: the engine's masked reset is what reset_envs is made of)
        env.engine.env_reset(mask=copies.repeat_interleave(env.num_possible_agents))


def hand_loop(env, policy, k, step0=0, done=None, opponent=None):
    """What a user writes today, through the façade, with pf_world_sync's rules restated on the host."""
    eng, E, A = env.engine, env.num_envs, env.num_possible_agents
    n, W = E * A, eng.action_dim
    done = torch.zeros(n, dtype=torch.bool, device=DEV) if done is None else done.clone()
    team1 = torch.as_tensor(env.team_flag, device=DEV).repeat(E) if opponent is not None else None
    out = {name: [] for name in ("obs", "actions", "mean", "reward", "terminated", "truncated", "valid")}
    for s in range(k):
        was = done.clone()
        waiting = was.view(E, A).all(dim=1)
        a, m = torch.empty(n, W, device=DEV), torch.empty(n, W, device=DEV)
        eng.policy_act(policy, step0 + s, out=a, mean_out=m)
        if opponent is not None:
            a = torch.where(team1[:, None], eng.policy_act(opponent, step0 + s), a)
        env.step({ag: a.view(E, A, W)[:, i] for i, ag in enumerate(env.possible_agents)})
        r, t, u = eng.reward.clone(), eng.terminated.clone(), eng.truncated.clone()
        ended = ~was & (t | u)
        out["reward"].append(torch.where(was, torch.zeros_like(r), r))
        out["terminated"].append(t & ~was)
        out["truncated"].append(u & ~was)
        out["valid"].append(~was if team1 is None else ~was & ~team1)
        if bool(waiting.any()):
            reset_copies(env, waiting)
        done = torch.where(waiting.repeat_interleave(A), torch.zeros_like(was), was | ended)
        out["obs"].append(eng.obs.clone())
        out["actions"].append(a)
        out["mean"].append(m)
    return {name: torch.stack(v) for name, v in out.items()}, done


def preconditions(t, E, A, k):
    """What makes the comparison mean something, asserted on the trajectory itself."""
    valid, ended = t["valid"].view(k, E, A), (t["terminated"] | t["truncated"]).view(k, E, A)
    share = float(valid.float().mean())
    first = torch.where(ended.any(dim=0), ended.float().argmax(dim=0), torch.full((E, A), -1, device=DEV))  # each agent's first ending step
    different = int(((first.max(dim=1).values != first.min(dim=1).values) & (first.min(dim=1).values >= 0)).sum())
    reset_step = ~valid.any(dim=2)  # [k, E]: no lane of the copy is valid -- its reset step
    again = 0
    for e in range(E):
        for s in torch.nonzero(reset_step[:, e]).flatten().tolist():
            if s < k - 1 and bool(valid[s + 1:, e].any()):
                again += 1
    truncations = int(t["truncated"].sum())
    print(f"valid share {share:.3f}, copies whose agents ended at different steps {different}, resets followed by valid steps {again}, "
          f"truncations {truncations}, terminations {int(t['terminated'].sum())}")
    assert different >= 1 and again >= 1 and truncations >= 1 and 0.5 < share < 1.0


NAMES = ("obs", "reward", "terminated", "truncated", "actions", "valid", "mean")
_cache = {}


def rollout_and_hand(kind):
    """The device rollout and the hand-written loop of one env kind, computed once and shared (nothing modifies them)."""
    if kind not in _cache:
        env1, env2 = make_env(kind), make_env(kind)
        k = DF_K if kind[0] == "dogfight" else HV_K
        policy = env_policy(env1)
        dev = dict(zip(NAMES, (x.clone() for x in env1.rollout(policy, k, store_mean=True))))
        hand, done = hand_loop(env2, policy, k)
        torch.cuda.synchronize()
        _cache[kind] = dict(dev=dev, hand=hand, hand_done=done, state1=env1.engine.state.clone(), state2=env2.engine.state.clone(),
                            latch1=env1.engine.world_done.clone(), agents1=list(env1.agents), E=env1.num_envs, A=env1.num_possible_agents, k=k)
        env1.close()
        env2.close()
    return _cache[kind]


# (team_size, num_envs): n = 64 and 66 -- worlds of six do not tile a wavefront; (shared_world,)
KINDS = [("dogfight", 2, 16), ("dogfight", 3, 11), ("hover", False), ("hover", True)]


# ---------------------------------------------------------------------------------------------- 1, 2. the loop is what it says
@pytest.mark.parametrize("kind", KINDS, ids=lambda k: "-".join(map(str, k)))
def test_rollout_is_the_hand_written_loop(kind):
    c = rollout_and_hand(kind)
    preconditions(c["dev"], c["E"], c["A"], c["k"])
    for name in NAMES:
        assert torch.equal(c["dev"][name], c["hand"][name]), name
    assert torch.equal(c["state1"], c["state2"])
    assert torch.equal(c["latch1"].bool(), c["hand_done"])
    assert len(c["agents1"]) == c["A"]


# ---------------------------------------------------------------------------------------------- 3. carry over calls
@pytest.mark.parametrize("kind", [("dogfight", 2, 16), ("hover", True)], ids=lambda k: "-".join(map(str, k)))
def test_two_calls_are_one(kind):
    # (the first call ends with the step that truncates whoever is still in the air: the dogfight's 32nd step, the hover's 22nd)
    half = 32 if kind[0] == "dogfight" else 22
    env1, env2 = make_env(kind), make_env(kind)
    policy = env_policy(env1)
    E, A = env1.num_envs, env1.num_possible_agents
    whole = [x.clone() for x in env1.rollout(policy, 2 * half, store_mean=True)]
    first = [x.clone() for x in env2.rollout(policy, half, store_mean=True)]
    waiting = env2.engine.world_done.view(E, A).bool().all(dim=1).clone()
    second = [x.clone() for x in env2.rollout(policy, half, store_mean=True)]
    assert bool(waiting.any())  # copies whose last agent finished in the first call's last step
    valid2 = second[NAMES.index("valid")].view(half, E, A)
    assert not bool(valid2[0, waiting].any()) and bool(valid2[1, waiting].all())  # reset in the second call's first step, flying in its second
    for name, w, a, b in zip(NAMES, whole, first, second):
        assert torch.equal(w, torch.cat((a, b))), name
    assert torch.equal(env1.engine.state, env2.engine.state) and torch.equal(env1.engine.world_done, env2.engine.world_done)
    env1.close()
    env2.close()


# ---------------------------------------------------------------------------------------------- 4. collect's batch
def host_gae(reward, terminated, truncated, values, valid, gamma, lam):
    """float64, lane by lane over the valid runs: between two consecutive valid steps the recursion continues unless the episode ended;
    behind a run's last step it is cut. (gamma and lambda as the float32 numbers the library receives.)"""
    k, n = reward.shape
    g, l = float(np.float32(gamma)), float(np.float32(lam))
    adv = np.zeros((k, n))
    for i in range(n):
        nxt, nxt_valid = 0.0, False
        for s in reversed(range(k)):
            if not valid[s, i]:
                nxt, nxt_valid = 0.0, False
                continue
            done = terminated[s, i] or truncated[s, i]
            delta = float(reward[s, i]) + g * (0.0 if terminated[s, i] else float(values[s + 1, i])) - float(values[s, i])
            adv[s, i] = delta + g * l * (nxt if (nxt_valid and not done) else 0.0)
            nxt, nxt_valid = adv[s, i], True
    return adv


@pytest.mark.parametrize("kind", [("dogfight", 3, 11), ("hover", False)], ids=lambda k: "-".join(map(str, k)))
def test_collect_batch(kind):
    env = make_env(kind)
    eng, k = env.engine, DF_K if kind[0] == "dogfight" else HV_K
    D, W, n = eng.obs_dim, eng.action_dim, eng.n
    torch.manual_seed(3)
    nn = torch.nn
    actor = nn.Sequential(nn.Linear(D, 32), nn.Tanh(), nn.Linear(32, W)).to(DEV)
    critic = nn.Sequential(nn.Linear(D, 32), nn.Tanh(), nn.Linear(32, 1)).to(DEV)
    log_std = nn.Parameter(torch.zeros(W, device=DEV))
    if kind[0] == "hover":
        actor[-1].weight.data *= 0.3
        actor[-1].bias.data.copy_(torch.tensor([0.0, 0.0, 0.0, HV_THRUST_BIAS]))
    policy = MLPPolicy.from_torch(actor, log_std=log_std)
    gamma, lam = 0.99, 0.95
    b = env.collect(policy, critic, k, gamma=gamma, lam=lam)
    assert set(b) == {"obs", "actions", "mean", "logp", "values", "advantages", "returns", "valid", "reward", "terminated", "truncated", "last_value", "infos"}
    assert tuple(b["obs"].shape) == (k, n, D) and tuple(b["valid"].shape) == (k, n) and b["valid"].dtype == torch.bool
    preconditions(b, env.num_envs, env.num_possible_agents, k)
    valid, term, trunc = (b[x].cpu().numpy() for x in ("valid", "terminated", "truncated"))
    reward = b["reward"].cpu().numpy()
    values = torch.cat((b["values"], b["last_value"][None])).cpu().numpy()
    with torch.no_grad():  # (values are the critic's on the k + 1 rows: obs is a view of them)
        assert torch.equal(b["values"], critic(b["obs"].reshape(k * n, D)).view(k, n))
    open_step = valid[:-1] & ~(term | trunc)[:-1]
    assert not (open_step & ~valid[1:]).any()  # a valid step that did not end its episode is followed by a valid step (except at row k - 1)
    ref = host_gae(reward, term, trunc, values, valid, gamma, lam)
    bound = gae_bound(gamma, lam, k, reward, values)
    adv, ret = b["advantages"].cpu().numpy().astype(np.float64), b["returns"].cpu().numpy().astype(np.float64)
    err_a, err_r = np.abs(adv - ref)[valid].max(), np.abs(ret - (ref + values[:-1]))[valid].max()
    print(f"advantages: max error {err_a:.3e}, returns {err_r:.3e}, bound {bound:.3e}")
    assert err_a <= bound and err_r <= bound
    want = torch.distributions.Normal(b["mean"].double(), log_std.detach().double().exp()).log_prob(b["actions"].double()).sum(-1)
    err_l, lb = float((b["logp"].double() - want).abs().max()), logp_bound(log_std.detach().cpu().numpy(), A=W)
    print(f"logp: max error {err_l:.3e}, bound {lb:.3e}")
    assert err_l <= lb
    o = b["obs"].reshape(k * n, D)
    loss, stats = pyflyt_amd.ppo_loss(env, actor(o), log_std, critic(o), b)
    loss.backward()
    assert float(stats[0]) == float(b["valid"].sum()) and bool(torch.isfinite(loss))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in list(actor.parameters()) + list(critic.parameters()) + [log_std])
    env.close()


# ---------------------------------------------------------------------------------------------- 5. the opponent
def test_opponent():
    kind = ("dogfight", 2, 16)
    k = 34  # (past the truncation and the resets behind it)
    env = make_env(kind)
    eng, E, A = env.engine, env.num_envs, env.num_possible_agents
    policy, other = env_policy(env, seed=5), env_policy(env, seed=6)
    team1 = torch.as_tensor(env.team_flag, device=DEV).repeat(E)
    obs0 = eng.obs.clone()
    t = dict(zip(NAMES, (x.clone() for x in env.rollout(policy, k, opponent=other, store_mean=True))))
    mine, theirs = eng.policy_act(policy, 0, obs=obs0).clone(), eng.policy_act(other, 0, obs=obs0).clone()
    assert torch.equal(t["actions"][0][team1], theirs[team1]) and torch.equal(t["actions"][0][~team1], mine[~team1])
    assert not torch.equal(mine[team1], theirs[team1])
    assert not bool(t["valid"][:, team1].any()) and bool(t["valid"][:, ~team1].any())
    env.close()
    # the same weights on both sides: the run without an opponent, but for valid
    env1, env2 = make_env(kind), make_env(kind)
    policy, twin = env_policy(env1, seed=5), env_policy(env1, seed=5)
    a = dict(zip(NAMES, (x.clone() for x in env1.rollout(policy, k, store_mean=True))))
    b = dict(zip(NAMES, (x.clone() for x in env2.rollout(policy, k, opponent=twin, store_mean=True))))
    for name in NAMES:
        if name != "valid":
            assert torch.equal(a[name], b[name]), name
    assert torch.equal(a["valid"] & ~team1, b["valid"]) and not torch.equal(a["valid"], b["valid"])
    assert torch.equal(env1.engine.state, env2.engine.state)
    env1.close()
    env2.close()


# ---------------------------------------------------------------------------------------------- 6. the façade after a collect
def test_facade_after_a_collect():
    env = make_env(("dogfight", 2, 16))
    E, A = env.num_envs, env.num_possible_agents
    policy = env_policy(env)
    critic = torch.nn.Linear(env.engine.obs_dim, 1).to(DEV)
    k = 20  # (before the truncation: some aircraft have left the dome, no copy has been reset in the last steps)
    b = env.collect(policy, critic, k)
    ended = (b["terminated"] | b["truncated"]).view(k, E, A)
    assert env.done.dtype == torch.bool and tuple(env.done.shape) == (E, A)
    assert torch.equal(env.done, env.engine.world_done.view(E, A).bool())
    assert bool(env.done.any()) and not bool(env.done.all())
    assert env.agents == env.possible_agents and env.step_count == k
    before = env.done.clone()
    # the latch is what the trajectory says: ended since the copy's last reset step (the step on which no lane of the copy is valid)
    valid, latch = b["valid"].view(k, E, A), torch.zeros(E, A, dtype=torch.bool, device=DEV)
    for s in range(k):
        latch = torch.where(~valid[s].any(dim=1, keepdim=True), torch.zeros_like(latch), latch | ended[s])
    assert torch.equal(before, latch)
    zero = {ag: torch.zeros(E, 4, device=DEV) for ag in env.possible_agents}
    env.step(zero)  # step() latches on top of it: nothing comes unlatched ...
    assert bool((env.done | ~before).all())
    for _ in range(31):  # ... and the 32nd step of an episode truncates whoever is left
        env.step(zero)
    assert bool(env.done.all()) and torch.equal(env.done, env.engine.world_done.view(E, A).bool())
    mask = torch.zeros(E, dtype=torch.bool, device=DEV)
    mask[::2] = True
    env.reset_envs(mask)
    assert not bool(env.done[mask].any()) and bool(env.done[~mask].all()) and env.agents == env.possible_agents
    env.close()


@pytest.mark.parametrize("kind", [("dogfight", 2, 16), ("hover", True)], ids=lambda k: "-".join(map(str, k)))
def test_partial_reset_after_a_rollout(kind):
    """rollout(k), a reset of SOME copies, rollout again: the copies that were not reset go on from the rollout's last row -- in what the
    reset returns, in the engine's current observation and in what the next rollout does, which is the hand-written loop's."""
    k, k2 = (20 if kind[0] == "dogfight" else 21), 16  # (agents have ended, no episode has been truncated yet)
    env1, env2 = make_env(kind), make_env(kind)
    policy = env_policy(env1)
    E, A, D = env1.num_envs, env1.num_possible_agents, env1.engine.obs_dim
    last = env1.rollout(policy, k)[0][k - 1].clone()
    latch = env1.engine.world_done.bool().clone()
    with_finished = torch.nonzero(latch.view(E, A).any(dim=1)).flatten()
    assert len(with_finished) >= 2 and not bool(latch.view(E, A).all(dim=1).all())
    copies = torch.zeros(E, dtype=torch.bool, device=DEV)
    copies[with_finished[::2]] = True  # every second copy that has finished agents, and every third of all
    copies[::3] = True
    copies[with_finished[1]] = False
    lanes = copies.repeat_interleave(A)
    assert bool(latch[lanes].any()) and bool(latch[~lanes].any())  # finished agents among the copies that are reset and among the others
    if kind[0] == "dogfight":
        got = env1.reset_envs(copies)
        returned = torch.stack([got[ag] for ag in env1.possible_agents], dim=1).reshape(E * A, D)
    else:
        returned = env1.engine.env_reset(mask=lanes)
    for name, obs in (("returned", returned), ("current", env1.engine._cur_obs)):
        assert torch.equal(obs[~lanes], last[~lanes]), name
        assert not torch.equal(obs[lanes], last[lanes]), name
    assert not bool(env1.engine.world_done[lanes].any()) and torch.equal(env1.engine.world_done.bool()[~lanes], latch[~lanes])
    second = dict(zip(NAMES, (x.clone() for x in env1.rollout(policy, k2, store_mean=True))))
    _, done = hand_loop(env2, policy, k)
    assert torch.equal(done, latch)
    reset_copies(env2, copies)
    hand, done = hand_loop(env2, policy, k2, step0=k, done=done & ~lanes)
    for name in NAMES:
        assert torch.equal(second[name], hand[name]), name
    assert torch.equal(env1.engine.state, env2.engine.state) and torch.equal(env1.engine.world_done.bool(), done)
    env1.close()
    env2.close()


# ---------------------------------------------------------------------------------------------- 7. the example
def test_selfplay_example():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "12_ppo_dogfight_selfplay.py"), "64", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("iteration")]
    assert len(lines) == 2 and all("valid share" in l and "reward per valid step" in l for l in lines), r.stdout

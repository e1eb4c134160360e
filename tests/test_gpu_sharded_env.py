"""make_vec(..., devices=[...]) -> ShardedVecEnv on the device, against the ONE vector env it is cut from: the shards reproduce it lane for
lane and bit for bit (steps, resets, rollouts, collect); with stats the running normalisers are those of all shards and every shard's
reward is scaled by the same number; one collect -> ppo_grad_sharded -> Adam.step lands where the single env's loop lands, within the
float32 tolerance of the gradient taken through the step; examples/19 runs. The two-device variants need two devices and are skipped
without them (two shards on one device run everywhere: one engine and its own buffers per shard either way)."""
import copy
import os
import subprocess
import sys

import pytest
import torch

import pyflyt_amd
from pyflyt_amd import Adam, MLPPolicy, Replicas, mlp, ppo_grad, ppo_grad_sharded
from pyflyt_amd.gym_envs import make_vec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOVER, FIXEDWING = "PyFlyt/QuadX-Hover-v4", "PyFlyt/Fixedwing-Waypoints-v4"
ONE, TWO = ["cuda:0", "cuda:0"], ["cuda:0", "cuda:1"]
DEVICE_LISTS = [ONE, pytest.param(TWO, marks=pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two devices"))]
KW = dict(seed=11, max_duration_seconds=1.0)


def networks(D, A=4, seed=3):
    torch.manual_seed(seed)
    nn = torch.nn
    actor = nn.Sequential(nn.Linear(D, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, A)).to("cuda:0")
    critic = nn.Sequential(nn.Linear(D, 64), nn.Tanh(), nn.Linear(64, 1)).to("cuda:0")
    return actor, critic, nn.Parameter(torch.full((A,), -0.5, device="cuda:0"))


def joined(parts, dim=0):
    return torch.cat([p.to("cuda:0") for p in parts], dim=dim)


@pytest.mark.parametrize("env_id, n, devices", [(HOVER, 256, ONE), (FIXEDWING, 256, ONE), (HOVER, 200, ["cuda:0"] * 3),
                                                pytest.param(HOVER, 256, TWO, marks=pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two devices"))])
def test_shards_reproduce_the_one_env(env_id, n, devices):
    kw = dict(KW, flatten=True) if env_id == FIXEDWING else KW  # (step()'s observation as one tensor)
    one, cut = make_vec(env_id, n, **kw), make_vec(env_id, n, devices=devices, **kw)
    try:
        assert [s.num_envs for s in cut.shards] == ([67, 67, 66] if n == 200 else [128, 128]) and cut.devices == [torch.device(d) for d in devices]
        obs, _ = one.reset(seed=11)
        obs_g, _ = cut.reset(seed=11)
        assert torch.equal(joined(obs_g), obs)
        ended = 0
        for step in range(40):  # (a second at 40 / 30 Hz: every lane is truncated and reset inside these steps)
            a, a_g = one.sample_actions(step), cut.sample_actions(step)
            assert torch.equal(joined(a_g), a)
            o, r, te, tr, _ = one.step(a)
            og, rg, teg, trg, _ = cut.step(a_g)
            for whole, parts in ((o, og), (r, rg), (te, teg), (tr, trg)):
                assert torch.equal(joined(parts), whole), step
            ended += int((te | tr).sum())
        assert ended >= n // 2  # (resets included)
        actor, _, log_std = networks(one.engine.obs_dim)
        rep = Replicas(dict(actor=actor, log_std=log_std), cut.devices)
        policy = MLPPolicy.from_torch(actor, log_std=log_std)
        policies = [MLPPolicy.from_torch(rep[g]["actor"], log_std=rep[g]["log_std"]) for g in range(len(devices))]
        whole, parts = one.rollout(policy, 40), cut.rollout(policies, 40)
        for i in range(5):  # obs, reward, terminated, truncated, actions: [k, n, ...]
            assert torch.equal(joined([p[i] for p in parts], dim=1), whole[i]), i
        assert bool((whole[2] | whole[3]).any())
    finally:
        one.close()
        cut.close()


BATCH_KEYS = ("obs", "actions", "mean", "logp", "values", "advantages", "returns", "valid", "reward", "terminated", "truncated")


@pytest.fixture(scope="module")
def pair():
    """The one env, the same env in two shards on one device, the networks and the policies: reset, nothing stepped."""
    one, cut = make_vec(HOVER, 256, **KW), make_vec(HOVER, 256, devices=ONE, **KW)
    obs, _ = one.reset(seed=11)
    cut.reset(seed=11)
    actor, critic, log_std = networks(obs.shape[1])
    policy = MLPPolicy.from_torch(actor, log_std=log_std)
    yield one, cut, actor, critic, log_std, policy
    one.close()
    cut.close()


def test_collect_gives_the_one_envs_slices(pair):
    one, cut, actor, critic, log_std, policy = pair
    b = one.collect(policy, lambda o: mlp(one, o, critic), 48)
    bs = cut.collect([policy] * 2, [lambda o, s=s: mlp(s, o, critic) for s in cut.shards], 48)
    for k in BATCH_KEYS:
        assert torch.equal(joined([x[k] for x in bs], dim=1), b[k]), k
    assert torch.equal(joined([x["last_value"] for x in bs]), b["last_value"])
    assert bool(b["valid"].any()) and not bool(b["valid"].all()) and bool((b["terminated"] | b["truncated"]).any())


def test_collect_with_stats_uses_the_normalisers_of_all_shards(pair):
    one, cut, actor, critic, log_std, policy = pair
    for s in [one] + cut.shards:  # (the episode accounting sees only collect(stats=True)'s steps: start it on fresh episodes)
        s.reset(seed=11)
    seen = 0.0
    for call in range(2):  # (the second call merges into the previous global blocks)
        b = one.collect(policy, lambda o: mlp(one, o, critic), 48, stats=True, normalize_reward=True)
        bs = cut.collect([policy] * 2, [lambda o, s=s: mlp(s, o, critic) for s in cut.shards], 48, stats=True, normalize_reward=True)
        ret, obs = cut.ret_rms.block, cut.obs_rms.block
        seen += float(b["valid"].sum())  # the valid steps so far: the count of both normalisers
        scale = 1.0 / (cut.ret_rms.var + 1e-8).sqrt()
        assert scale.numel() == 1 and float(scale) != 1.0
        for s, x in zip(cut.shards, bs):
            assert torch.equal(s.ret_rms.block, ret) and torch.equal(s.obs_rms.block, obs)  # one number on all shards
            assert torch.equal(x["reward_scaled"], x["reward"] / (cut.ret_rms.var + 1e-8).sqrt().to(x["reward"].device))
        for name, got, want in (("ret", ret, one.ret_rms.block), ("obs", obs, one.obs_rms.block)):
            big = max(float(want.abs().max()), float(got.abs().max()))
            err = float((got - want).abs().max())
            print(f"call {call} {name}_rms: max error {err:.3e} = {err / (2.0 ** -52 * big):.2f} ulps of the largest entry {big:.3e}")
            assert float(got[0]) == float(want[0]) == seen
            assert err <= 64 * 2.0 ** -52 * big, (name, err, big)
        for k in ("obs", "actions", "reward", "terminated", "truncated", "valid", "episode_length"):
            assert torch.equal(joined([x[k] for x in bs], dim=1), b[k]), k
        d1, dg = one.episode_summary_dict(), cut.episode_summary_dict()
        for k in ("episodes", "terminated", "truncated", "return_min", "return_max"):
            assert d1[k] == dg[k], k
        assert d1["episodes"] >= 128
        N, top = d1["episodes"], max(abs(d1["return_min"]), abs(d1["return_max"]))
        assert abs(d1["return_mean"] - dg["return_mean"]) <= N * 2.0 ** -52 * top
        assert abs(d1["length_mean"] - dg["length_mean"]) <= N * 2.0 ** -52 * 48
        assert abs(d1["return_std"] - dg["return_std"]) <= 4 * N * 2.0 ** -52 * top * top / max(d1["return_std"], 1e-300)


@pytest.mark.parametrize("devices", DEVICE_LISTS)
def test_one_iteration_lands_where_the_one_envs_loop_lands(devices):
    K, LR, EPS = 32, 3e-4, 1e-8
    coef = dict(clip=0.2, vf_coef=1.0, ent_coef=0.0, normalize_advantage=True, clip_vf=0.2, bounds_coef=1e-4)
    one, cut = make_vec(HOVER, 256, **KW), make_vec(HOVER, 256, devices=devices, **KW)
    try:
        obs, _ = one.reset(seed=11)
        cut.reset(seed=11)
        D = obs.shape[1]
        actor, critic, log_std = networks(D)
        a2, c2, l2 = copy.deepcopy(actor), copy.deepcopy(critic), torch.nn.Parameter(log_std.detach().clone())
        bounds = (one.single_action_space.low, one.single_action_space.high)
        # example 18's iteration on the one env: a batch, the gradient of all its rows, a step
        policy = MLPPolicy.from_torch(actor, log_std=log_std)
        p1 = list(actor.parameters()) + list(critic.parameters()) + [log_std]
        o1 = Adam(one, p1, lr=LR, eps=EPS, max_grad_norm=0.5)
        with torch.no_grad():
            b = one.collect(policy, lambda o: mlp(one, o, critic), K, stats=True, normalize_reward=True)
        before = [p.detach().clone() for p in p1]
        ppo_grad(one, b["obs"].reshape(-1, D), actor, critic, log_std, b, action_bounds=bounds, **coef)
        g1 = [p.grad.clone() for p in p1]
        o1.step()
        clip1 = o1.stats_dict()["clip_coef"]
        # example 19's on the shards
        rep = Replicas(dict(actor=a2, critic=c2, log_std=l2), cut.devices)
        policies = [MLPPolicy.from_torch(rep[g]["actor"], log_std=rep[g]["log_std"]) for g in range(2)]
        p2 = list(a2.parameters()) + list(c2.parameters()) + [l2]
        o2 = Adam(cut.shards[0], p2, lr=LR, eps=EPS, max_grad_norm=0.5)
        with torch.no_grad():
            bs = cut.collect(policies, [lambda o, g=g: mlp(cut.shards[g], o, rep[g]["critic"]) for g in range(2)], K, stats=True, normalize_reward=True)
        stats = ppo_grad_sharded(cut, [x["obs"].reshape(-1, D) for x in bs], rep, bs, action_bounds=bounds, **coef)
        g2 = [p.grad.clone() for p in p2]
        o2.step()
        rep.sync()
        torch.cuda.synchronize()
        for g in range(2):  # the copies are the masters' again
            for name in ("actor", "critic"):
                for u, v in zip(rep[g][name].parameters(), rep[0][name].parameters()):
                    assert torch.equal(u.to("cuda:0"), v)
            assert torch.equal(rep[g]["log_std"].to("cuda:0"), l2)
        assert float(stats[0]) == float(b["valid"].sum()) and abs(clip1 - o2.stats_dict()["clip_coef"]) <= 1e-5 * clip1
        # the project's float32 tolerance for the gradient, 8 * 2^-24 max |g| per tensor, taken through the first Adam step
        # p - lr u(g'), u = g' / (|g'| + eps), g' the clipped gradient: |du/dg'| = eps / (|g'| + eps)^2, and u never moves by more than 2
        worst = 0.0
        for name, u, v, p0, ga, gb in zip(range(len(p1)), p1, p2, before, g1, g2):
            tol_g = 2.0 * 8.0 * 2.0 ** -24 * float(ga.abs().max())  # (either path within the tolerance of the exact gradient)
            assert float((ga - gb).abs().max()) <= tol_g, (name, float((ga - gb).abs().max()), tol_g)
            gc = ga.abs().double() * clip1
            moved = torch.clamp(EPS * (tol_g * clip1 + 1e-5 * gc) / (gc + EPS) ** 2, max=2.0)
            bound = LR * moved + 4.0 * 2.0 ** -24 * (p0.abs().double() + LR)
            ratio = float(((u.detach().double() - v.detach().double()).abs() / bound).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (name, ratio)
            assert not torch.equal(u.detach(), p0)  # (a step was taken)
        print(f"devices {devices}: the largest |p_sharded - p_single| / bound after one step: {worst:.3f}")
    finally:
        one.close()
        cut.close()


def test_example_19_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "19_ppo_sharded.py"), "256", "2"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("iter")]
    assert len(lines) == 2 and "2 shards" in lines[0] and "nan" not in out.stdout.lower() and "inf" not in out.stdout.lower()

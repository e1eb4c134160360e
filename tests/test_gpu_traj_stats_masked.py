"""pf_traj_stats_masked and the multi-agent collect(stats=True) on the device. The reference is test_gpu_traj_stats.ref_traj with its
validity line replaced by the given mask (ref_masked below: the flags, reward and observation of an invalid step are ignored); every
tolerance is one of the bounds derived in test_gpu_traj_stats.py. Synthetic masks, NaN poisoning of everything that must not be
selected, bit equivalence with pf_traj_stats, splitting, graph capture, the C ABI's error paths, collect end to end on both
multi-agent envs, resets, the example.

The end-to-end trajectories are those of test_gpu_ma_collect.py (DF_KW / HV_KW, its env and policy builders; its header says what was
checked on the fp64 oracle: agents of one copy ending at different steps, terminations and truncations, valid share 0.64-0.80). An
episode's last possible step is the truncating one, step max_steps + 2 of the episode (`step_count > max_steps` after the step's
increment: the dogfight's 32nd, the hover's 22nd -- test_gpu_ma_collect.test_two_calls_are_one). Two whole episodes and the reset step
between them are 65 steps on the dogfight and 45 on the hover, so k = 66 and 48: every trained lane finishes two episodes whatever the
policy does. (64 steps would be one short for an aircraft that flies to the truncation twice.)"""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from pyflyt_amd import _lib as L
from pyflyt_amd import build_params
from pyflyt_amd.engine import BatchEngine
from test_gpu_ma_collect import DF_KW, HV_KW, KINDS, env_policy, make_env  # noqa: F401 (DF_KW / HV_KW: what make_env builds with)
from test_gpu_traj_stats import (N, check_lanes, check_moments, check_summary, dev, engine, fma32, moments_bound, ref_traj, same_bits,
                                 synth)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 21
STATE = ("carry_return", "carry_length", "carry_disc")
OUT = ("ep_ret", "ep_len", "summary", "ret_moments", "obs_moments")


# ---------------------------------------------------------------------------------------------- the reference
def ref_masked(gamma, reward, terminated, truncated, valid, carry=None):
    """test_gpu_traj_stats.ref_traj with `v = valid[s]` as its validity line: the same float32 recursion, sequential in s."""
    k, n = reward.shape
    g = np.float32(gamma)
    ret, ln, G = (x.copy() for x in carry) if carry is not None else (np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.float32))
    term, trunc, valid = terminated.astype(bool), truncated.astype(bool), valid.astype(bool)
    ep_ret, ep_len = np.zeros((k, n), np.float32), np.zeros((k, n), np.int32)
    Gs, fins = np.zeros((k, n), np.float32), np.zeros((k, n), dtype=bool)
    with np.errstate(invalid="ignore"):
        for s in range(k):
            done, v = term[s] | trunc[s], valid[s]
            ret = np.where(v, (ret + reward[s]).astype(np.float32), ret)
            ln = np.where(v, ln + 1, ln).astype(np.int32)
            G = np.where(v, fma32(g, G, reward[s]), G)
            Gs[s] = G
            fin = v & done
            fins[s] = fin
            ep_ret[s], ep_len[s] = np.where(fin, ret, np.float32(0)), np.where(fin, ln, 0)
            ret, ln, G = np.where(fin, np.float32(0), ret), np.where(fin, 0, ln).astype(np.int32), np.where(fin, np.float32(0), G)
    r64 = ep_ret[fins].astype(np.float64)
    c = int(fins.sum())
    summary = np.array([c, r64.sum(), (r64 * r64).sum(), r64.min() if c else np.inf, r64.max() if c else -np.inf, ep_len[fins].sum(),
                        (fins & term).sum(), (fins & ~term).sum()], dtype=np.float64)
    return dict(ep_ret=ep_ret, ep_len=ep_len, valid=valid, G=Gs, fin=fins, carry=(ret, ln, G), summary=summary)


def masked_synth(k, n=N, seed=0):
    """Random rewards, flags with probability 0.06 each on EVERY step (valid or not), a mask of about 70 % ones, and the lanes the
    contract is about: 0 never valid, 1 always, 2 invalid at s = 0, 3 invalid at s = k - 1, 4 invalid over s = 11..17 (across the edge
    of a 12-step and of a 16-step window) between two valid steps, 5 two episodes with invalid steps -- flags set -- between them."""
    rng = np.random.default_rng(1000 + 31 * k + seed)
    term, trunc = rng.random((k, n)) < 0.06, rng.random((k, n)) < 0.06
    valid = rng.random((k, n)) < 0.7
    reward = (rng.normal(size=(k, n)) * 2.0 + 0.5).astype(np.float32)
    obs = (rng.normal(size=(k, n, D)) * np.linspace(0.1, 3.0, D) + np.linspace(-2.0, 5.0, D)).astype(np.float32)
    valid[:, 0], valid[:, 1] = False, True
    term[k // 2, 0] = True  # (a flag on the lane that is never valid)
    valid[0, 2] = valid[k - 1, 3] = False
    if k > 18:
        valid[10:19, 4] = [True] + [False] * 7 + [True]
    if k >= 6:
        valid[:6, 5] = [True, True, False, False, True, True]
        term[:6, 5] = [False, True, True, False, False, False]
        trunc[:6, 5] = [False, False, False, True, False, True]
    return dict(reward=reward, terminated=term, truncated=trunc, valid=valid, obs=obs)


def run(eng, d, gamma=0.99):
    """BatchEngine.traj_stats on the arrays of d -- masked where d has `valid`, pf_traj_stats otherwise -- and everything it left."""
    er, el, summ = eng.traj_stats(dev(d["reward"]), dev(d["terminated"]), dev(d["truncated"]), gamma=gamma, episode_start=dev(d.get("episode_start")),
                                  obs=dev(d.get("obs")), valid=dev(d.get("valid")))
    torch.cuda.synchronize()
    return left(eng, er, el, summ)


def left(eng, er, el, summ):
    ts = eng._traj_state()
    return dict(ep_ret=er.cpu().numpy().copy(), ep_len=el.cpu().numpy().copy(), summary=summ.cpu().numpy().copy(),
                carry=tuple(ts[key].cpu().numpy().copy() for key in STATE), ret_moments=ts["ret_moments"].cpu().numpy().copy(),
                obs_moments=ts["obs_moments"].cpu().numpy().copy())


def all_same_bits(a, b):
    for key in OUT:
        assert same_bits(a[key], b[key]), key
    for name, x, y in zip(STATE, a["carry"], b["carry"]):
        assert same_bits(x, y), name


def check_all(got, ref, d, rows):
    """Per-step outputs and carries bit for bit, summary and both moment blocks (empty before the call) within the derived bounds."""
    check_lanes(got, ref)
    check_summary(got, ref, rows)
    v, zero = ref["valid"], np.zeros(1)
    check_moments(got["ret_moments"], ref["G"][v][:, None], moments_bound(rows, ref["G"][v][:, None], zero, zero), "ret_moments")
    Dm = d["obs"].shape[-1]
    check_moments(got["obs_moments"], d["obs"][v], moments_bound(rows, d["obs"][v], np.zeros(Dm), np.zeros(Dm)), "obs_moments")


# ---------------------------------------------------------------------------------------------- 1. synthetic masks
@pytest.mark.parametrize("mode", ["off", "next_step"])
@pytest.mark.parametrize("k", [1, 7, 37])
def test_synthetic_masks(mode, k):
    d = masked_synth(k)
    v, done = d["valid"], d["terminated"] | d["truncated"]
    ref = ref_masked(0.99, d["reward"], d["terminated"], d["truncated"], v)
    # the inputs exercise the contract
    assert N == 200 and not v[:, 0].any() and v[:, 1].all() and not v[0, 2] and not v[k - 1, 3] and 0.6 < v[:, 6:].mean() < 0.8
    assert done[:, 0].any()  # (a flag on the lane that is never valid)
    if k > 18:
        assert v[10, 4] and v[18, 4] and not v[11:18, 4].any()
    if k >= 6:
        f = np.nonzero(ref["fin"][:, 5])[0]
        assert list(f[:2]) == [1, 5] and not v[2:4, 5].any() and done[2:4, 5].all()
        assert (done & ~v).sum() > 0 and (ref["fin"].sum(0) >= 2).any()
    eng = engine(mode)
    assert eng.obs_dim == D
    got = run(eng, d)
    assert not got["ep_ret"][:, 0].any() and not got["ep_len"][:, 0].any() and not any(c[0] for c in got["carry"])
    check_all(got, ref, d, k * N)
    eng.close()


# ---------------------------------------------------------------------------------------------- 2. poison
@pytest.mark.parametrize("mode", ["off", "next_step"])
@pytest.mark.parametrize("k", [7, 37])
def test_poison_in_invalid_steps_reaches_nothing(mode, k):
    d = masked_synth(k, seed=1)
    inv = ~d["valid"]
    assert inv.any() and d["valid"].any()
    p = {key: val.copy() for key, val in d.items()}
    p["reward"][inv] = np.nan
    p["obs"][inv] = np.nan
    p["terminated"][inv] = True
    p["truncated"][inv] = True
    e1, e2 = engine(mode), engine(mode)
    clean, dirty = run(e1, d), run(e2, p)
    all_same_bits(clean, dirty)
    for key in ("ep_ret", "ret_moments", "obs_moments") :
        assert np.isfinite(dirty[key]).all(), key
    assert np.isfinite(dirty["summary"][[0, 1, 2, 5, 6, 7]]).all() and all(np.isfinite(c).all() for c in dirty["carry"])
    assert dirty["summary"][0] > 0 and np.isfinite(dirty["summary"][3:5]).all()  # (episodes finished: min and max are returns)
    e1.close(); e2.close()


# ---------------------------------------------------------------------------------------------- 3. equivalence with pf_traj_stats
def equivalence(mode, k, n, seed):
    d = synth(mode, k, n=n, seed=seed, D=D)
    ref = ref_traj(mode, 0.99, d["reward"], d["terminated"], d["truncated"], d["episode_start"])
    if mode == "next_step":
        assert (~ref["valid"]).any() and d["episode_start"].any()
    else:
        assert ref["valid"].all()
    m = {key: val for key, val in d.items() if key != "episode_start"}
    m["valid"] = ref["valid"]  # (what pf_gae writes to valid_out: test_gpu_gae pins it to this rule; all ones under SAME_STEP)
    e1, e2 = engine(mode, n=n), engine(mode, n=n)
    a, b = run(e1, d), run(e2, m)
    all_same_bits(a, b)
    assert a["summary"][0] > 0 and a["obs_moments"][0] == ref["valid"].sum() and a["ret_moments"][0] == ref["valid"].sum()
    e1.close(); e2.close()


@pytest.mark.parametrize("mode", ["next_step", "same_step"])
@pytest.mark.parametrize("k", [1, 7, 37])
def test_same_bits_as_traj_stats(mode, k):
    equivalence(mode, k, N, 0)


@pytest.mark.parametrize("mode", ["next_step", "same_step"])
def test_same_bits_as_traj_stats_beyond_one_pass_of_the_grid(mode):
    """n = 4096, k = 37, D = 21: the observation kernel's eight-row loop and its tail both run
    (test_gpu_traj_stats.test_observation_moments_beyond_one_pass_of_the_grid)."""
    equivalence(mode, 37, 4096, 8)


def test_the_mask_of_gae_is_the_reference_mask():
    """pf_gae's valid_out on a NEXT_STEP trajectory, fed back as `valid`: the same bits as pf_traj_stats with the same episode_start."""
    k = 37
    d = synth("next_step", k, D=D)
    e1, e2 = engine("next_step"), engine("next_step")
    t = {key: dev(val) for key, val in d.items()}
    values = torch.zeros(k + 1, N, device=DEV)
    valid = e2.gae(t["reward"], t["terminated"], t["truncated"], values, episode_start=t["episode_start"])[3]
    assert valid.dtype == torch.bool and not bool(valid.all())
    a = run(e1, d)
    b = left(e2, *e2.traj_stats(t["reward"], t["terminated"], t["truncated"], gamma=0.99, obs=t["obs"], valid=valid))
    all_same_bits(a, b)
    e1.close(); e2.close()


# ---------------------------------------------------------------------------------------------- 4. splitting
def test_splitting_a_call():
    k, h = 36, 18
    d = masked_synth(k, seed=2)
    ref = ref_masked(0.99, d["reward"], d["terminated"], d["truncated"], d["valid"])
    whole, split = engine("off"), engine("off")
    w = run(whole, d)
    ga = run(split, {key: val[:h] for key, val in d.items()})
    mid = dict(obs_moments=ga["obs_moments"].copy(), ret_moments=ga["ret_moments"].copy())
    gb = run(split, {key: val[h:] for key, val in d.items()})
    assert same_bits(np.concatenate([ga["ep_ret"], gb["ep_ret"]]), w["ep_ret"]) and same_bits(w["ep_ret"], ref["ep_ret"])
    assert np.array_equal(np.concatenate([ga["ep_len"], gb["ep_len"]]), w["ep_len"]) and np.array_equal(w["ep_len"], ref["ep_len"])
    for x, y, z in zip(gb["carry"], w["carry"], ref["carry"]):
        assert same_bits(x, y) and same_bits(x, z)
    assert ga["summary"][0] + gb["summary"][0] == w["summary"][0] and min(ga["summary"][3], gb["summary"][3]) == w["summary"][3]
    v = ref["valid"]
    for name, samples in (("obs_moments", d["obs"]), ("ret_moments", ref["G"][..., None])):
        Dm = samples.shape[-1]
        allv, first, second = samples[v], samples[:h][v[:h]], samples[h:][v[h:]]
        bw = moments_bound(k * N, allv, np.zeros(Dm), np.zeros(Dm))
        b1 = moments_bound(h * N, first, np.zeros(Dm), np.zeros(Dm))
        b2 = moments_bound(h * N, second, mid[name][1:1 + Dm], mid[name][1 + Dm:])
        check_moments(w[name], allv, bw, name + " (one call)")
        check_moments(gb[name], allv, (b1[0] + b2[0], b1[1] + b2[1]), name + " (two calls)")
    whole.close(); split.close()


# ---------------------------------------------------------------------------------------------- 5. graph capture
def test_the_masked_call_is_capturable():
    k = 20
    t = {key: dev(val) for key, val in masked_synth(k, seed=6).items()}
    state = STATE + ("obs_moments", "ret_moments")

    def call(eng):
        return eng.traj_stats(t["reward"], t["terminated"], t["truncated"], gamma=0.99, obs=t["obs"], valid=t["valid"])

    twin = engine("off")
    call(twin)
    out2 = call(twin)
    torch.cuda.synchronize()
    eager = [x.clone() for x in out2] + [twin._traj_state()[key].clone() for key in state]
    eng = engine("off")
    ts = eng._traj_state()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # (the engine's first call makes its tensors: not inside the capture)
        call(eng)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call(eng)
    for x in out:
        x.zero_()
    for key in state:
        ts[key].zero_()
    torch.cuda.synchronize()
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(list(out) + [ts[key] for key in state], eager):
        assert same_bits(x.cpu().numpy(), y.cpu().numpy())
    assert float(ts["obs_moments"][0]) == 2 * float(t["valid"].sum()) > 0 and float(eager[0].abs().sum()) > 0
    eng.close(); twin.close()


# ---------------------------------------------------------------------------------------------- 6. error paths
def test_error_paths_name_the_argument():
    k, n = 4, 64
    for mode in ("next_step", "same_step", "off"):
        eng = engine(mode, n=n)
        f32, f64 = dict(dtype=torch.float32, device=DEV), dict(dtype=torch.float64, device=DEV)
        buf = dict(reward=torch.zeros(k, n, **f32), terminated=torch.zeros(k, n, dtype=torch.bool, device=DEV),
                   truncated=torch.zeros(k, n, dtype=torch.bool, device=DEV), valid=torch.ones(k, n, dtype=torch.bool, device=DEV),
                   obs=torch.zeros(k, n, D, **f32), carry_return=torch.zeros(n, **f32), carry_length=torch.zeros(n, dtype=torch.int32, device=DEV),
                   carry_disc=torch.zeros(n, **f32), ep_return_out=torch.zeros(k, n, **f32),
                   ep_length_out=torch.zeros(k, n, dtype=torch.int32, device=DEV), summary=torch.zeros(8, **f64),
                   ret_moments=torch.zeros(3, **f64), obs_moments=torch.zeros(1 + 2 * D, **f64))

        def block(**change):
            a = L.PfTrajStatsMasked()
            a.gamma = 0.99
            for key, v in {**buf, **change}.items():
                setattr(a, key, v if isinstance(v, float) or v is None else v.data_ptr())
            return a

        def refused(fragment, steps=k, **change):
            rc = eng.lib.pf_traj_stats_masked(eng._ctx, C.byref(block(**change)), steps, eng._stream())
            msg = eng.lib.pf_last_error(eng._ctx).decode()
            assert rc == L.ERR_ARG and fragment in msg and "pf_traj_stats_masked" in msg, (rc, msg)

        assert eng.lib.pf_traj_stats_masked(eng._ctx, C.byref(block()), k, eng._stream()) == 0  # (the unchanged block is accepted)
        assert eng.lib.pf_traj_stats_masked(eng._ctx, C.byref(block(ep_return_out=None, ep_length_out=None, ret_moments=None, obs=None, obs_moments=None)),
                                            k, eng._stream()) == 0  # (and so is one without anything optional)
        refused("k_steps", steps=0)
        for name in ("valid", "reward", "terminated", "truncated", "summary", "carry_return", "carry_length", "carry_disc"):
            refused(name, **{name: None})
        refused("gamma", gamma=1.5)
        refused("gamma", gamma=-0.5)
        refused("gamma", gamma=float("nan"))
        refused("obs comes with obs_moments", obs_moments=None)
        refused("obs_moments comes with obs", obs=None)
        torch.cuda.synchronize()
        with pytest.raises(ValueError, match="valid and episode_start do not come together"):
            eng.traj_stats(buf["reward"], buf["terminated"], buf["truncated"], episode_start=torch.zeros(n, dtype=torch.bool, device=DEV), valid=buf["valid"])
        eng.close()
    aviary = BatchEngine(build_params("quadx", "none"), 64, device=DEV)
    rc = aviary.lib.pf_traj_stats_masked(aviary._ctx, C.byref(L.PfTrajStatsMasked()), 4, aviary._stream())
    assert rc == L.ERR_UNSUPPORTED and "env task" in aviary.lib.pf_last_error(aviary._ctx).decode()
    aviary.close()


# ---------------------------------------------------------------------------------------------- 7. collect end to end
TODAYS_KEYS = {"obs", "actions", "mean", "logp", "values", "advantages", "returns", "valid", "reward", "terminated", "truncated", "last_value", "infos"}
STATS_KEYS = {"episode_return", "episode_length", "episode_summary"}
GAMMA = 0.99


def steps_for(kind):
    return 66 if kind[0] == "dogfight" else 48


def make_critic(env):
    torch.manual_seed(7)
    nn = torch.nn
    return nn.Sequential(nn.Linear(env.engine.obs_dim, 32), nn.Tanh(), nn.Linear(32, 1)).to(DEV)


def check_batch(env, b, k, excluded=None):
    """collect(stats=True)'s batch and what it left in the engine (empty before the call) against the masked reference on the batch's own
    reward, flags and valid. Returns the reference."""
    n, Dm = env.engine.n, env.engine.obs_dim
    rew, term, trunc, valid = (b[x].cpu().numpy() for x in ("reward", "terminated", "truncated", "valid"))
    ref = ref_masked(GAMMA, rew, term, trunc, valid)
    trained = np.ones(n, dtype=bool) if excluded is None else ~excluded
    per_lane = ref["fin"].sum(0)
    between = 0  # lanes with invalid steps between their first two episodes
    for i in np.nonzero(trained)[0]:
        f = np.nonzero(ref["fin"][:, i])[0]
        between += len(f) >= 2 and bool((~valid[f[0] + 1:f[1], i]).any())
    print(f"{int(ref['fin'].sum())} episodes, at least {int(per_lane[trained].min())} per trained lane, {between} lanes with invalid steps between two "
          f"episodes, {int((ref['fin'] & term).sum())} terminations, {int((ref['fin'] & ~term).sum())} truncations, valid share {valid.mean():.3f}")
    assert per_lane[trained].min() >= 2 and between >= 1
    assert (ref["fin"] & term).any() and (ref["fin"] & ~term & trunc).any()
    assert same_bits(b["episode_return"].cpu().numpy(), ref["ep_ret"]) and np.array_equal(b["episode_length"].cpu().numpy(), ref["ep_len"])
    assert b["episode_length"].dtype == torch.int32
    ts = env.engine._traj_state()
    got = dict(summary=b["episode_summary"].cpu().numpy(), carry=tuple(ts[key].cpu().numpy() for key in STATE))
    for name, x, y in zip(STATE, got["carry"], ref["carry"]):
        assert same_bits(x, y), name
    check_summary(got, ref, k * n)
    obs = b["obs"].cpu().numpy()
    check_moments(env.obs_rms.block.cpu().numpy(), obs[valid], moments_bound(k * n, obs[valid], np.zeros(Dm), np.zeros(Dm)), "obs_rms")
    G = ref["G"][valid][:, None]
    check_moments(env.ret_rms.block.cpu().numpy(), G, moments_bound(k * n, G, np.zeros(1), np.zeros(1)), "ret_rms")
    sd = env.episode_summary_dict()
    assert sd["episodes"] == int(ref["fin"].sum()) and sd["terminated"] == int((ref["fin"] & term).sum())
    assert sd["terminated"] + sd["truncated"] == sd["episodes"]
    assert math.isclose(sd["return_mean"], float(ref["ep_ret"][ref["fin"]].astype(np.float64).mean()), rel_tol=1e-9, abs_tol=1e-9)
    assert math.isclose(sd["length_mean"], float(ref["ep_len"][ref["fin"]].mean()), rel_tol=1e-12)
    assert sd["return_min"] == float(ref["ep_ret"][ref["fin"]].min()) and sd["return_max"] == float(ref["ep_ret"][ref["fin"]].max())
    return ref


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: "-".join(map(str, k)))
def test_collect_with_stats_end_to_end(kind):
    k = steps_for(kind)
    env, twin = make_env(kind), make_env(kind)
    n = env.engine.n
    policy, critic = env_policy(env), make_critic(env)
    b = env.collect(policy, critic, k, gamma=GAMMA, stats=True)
    torch.cuda.synchronize()
    assert set(b) == TODAYS_KEYS | STATS_KEYS
    check_batch(env, b, k)
    # a twin env's default call: today's keys, and the tensors this batch has -- nothing existing moved
    b0 = twin.collect(policy, critic, k, gamma=GAMMA)
    assert set(b0) == TODAYS_KEYS
    for key in TODAYS_KEYS - {"infos"}:
        assert torch.equal(b0[key], b[key]), key
    assert twin.engine.made_moments() is None
    # normalize_reward: pf_gae gets the scaled reward, computed with the moments AFTER this batch's update; reward stays raw
    count1 = float(env.ret_rms.count)
    b2 = env.collect(policy, critic, k, gamma=GAMMA, normalize_reward=True)
    assert set(b2) == TODAYS_KEYS | STATS_KEYS | {"reward_scaled"}
    assert torch.equal(b2["reward_scaled"], b2["reward"] / (env.ret_rms.var + 1e-8).sqrt())
    assert float(env.ret_rms.count) == count1 + float(b2["valid"].sum()) and not torch.equal(b2["reward_scaled"], b2["reward"])
    adv, ret = b2["advantages"].clone(), b2["returns"].clone()
    values = torch.cat([b2["values"], b2["last_value"][None]], 0).contiguous()
    a2, r2, _, _ = env.engine.gae(b2["reward_scaled"], b2["terminated"], b2["truncated"], values, gamma=GAMMA, lam=0.95)
    assert torch.equal(a2, adv) and torch.equal(r2, ret)
    assert tuple(b2["episode_return"].shape) == (k, n)
    env.close(); twin.close()


def test_collect_with_stats_and_an_opponent():
    kind = ("dogfight", 2, 16)
    k = steps_for(kind)
    env = make_env(kind)
    policy, other, critic = env_policy(env, seed=5), env_policy(env, seed=6), make_critic(env)
    team1 = torch.as_tensor(env.team_flag, device=DEV).repeat(env.num_envs)
    b = env.collect(policy, critic, k, gamma=GAMMA, opponent=other, stats=True)
    torch.cuda.synchronize()
    assert set(b) == TODAYS_KEYS | STATS_KEYS
    assert not bool(b["valid"][:, team1].any()) and bool((b["terminated"] | b["truncated"])[:, team1].any())  # (flags there, and no valid step)
    check_batch(env, b, k, excluded=team1.cpu().numpy())
    ts = env.engine._traj_state()
    for key in STATE:
        assert not bool(ts[key][team1].any()), key
    assert not bool(b["episode_return"][:, team1].any()) and not bool(b["episode_length"][:, team1].any())
    assert float(env.obs_rms.count) == float(b["valid"].sum()) == float(env.ret_rms.count)
    env.close()


# ---------------------------------------------------------------------------------------------- 8. resets
@pytest.mark.parametrize("kind", [("dogfight", 2, 16), ("hover", True)], ids=lambda k: "-".join(map(str, k)))
def test_resets_zero_the_carries_and_keep_the_moments(kind):
    env = make_env(kind)
    E, A = env.num_envs, env.num_possible_agents
    policy, critic = env_policy(env), make_critic(env)
    env.collect(policy, critic, 7, stats=True)  # (7 steps: most episodes are open)
    ts = env.engine._traj_state()
    before = {key: ts[key].clone() for key in STATE}
    assert (before["carry_length"] > 0).float().mean() > 0.5 and (before["carry_return"] != 0).float().mean() > 0.5
    moments = env.obs_rms.block.clone(), env.ret_rms.block.clone()
    assert 0 < float(moments[0][0]) <= 7 * E * A
    if kind[0] == "dogfight":  # (the hover façade has no per-copy reset)
        copies = torch.zeros(E, dtype=torch.bool, device=DEV)
        copies[3:9] = True
        lanes = copies.repeat_interleave(A)
        env.reset_envs(copies)
        for key, was in before.items():
            assert was[lanes].any() and not ts[key][lanes].any() and torch.equal(ts[key][~lanes], was[~lanes]), key
        assert torch.equal(env.obs_rms.block, moments[0]) and torch.equal(env.ret_rms.block, moments[1])
    env.reset(seed=12)  # another seed: a new engine
    assert env.engine._traj_state() is not ts and not any(env.engine._traj_state()[key].any() for key in STATE)
    assert torch.equal(env.obs_rms.block, moments[0]) and torch.equal(env.ret_rms.block, moments[1])
    env.collect(policy, critic, 7, stats=True)
    assert float(env.obs_rms.count) > float(moments[0][0])
    env.reset()  # the same engine: zero carries, the moments stay
    assert not any(env.engine._traj_state()[key].any() for key in STATE) and float(env.obs_rms.count) > float(moments[0][0])
    env.close()


# ---------------------------------------------------------------------------------------------- 9. the example
def test_example_14_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "14_ppo_dogfight_selfplay_stats.py"), "64", "2"], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr[-2000:]
    rows = re.findall(r"iteration \d+: (\d+) episodes finished, mean episode return ([-+0-9.eE]+|nan|inf), mean episode length ([-+0-9.eE]+|nan|inf), "
                      r"(\d+) terminated / (\d+) truncated", out.stdout)
    assert len(rows) == 2, out.stdout
    for episodes, ret, length, te, tr in rows:
        assert int(episodes) > 0 and math.isfinite(float(ret)) and float(length) > 0 and int(te) + int(tr) == int(episodes), out.stdout

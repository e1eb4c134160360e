"""pf_gae and env.collect on the device, against a float64 numpy restatement of the semantics in include/pyflyt_amd.h (written from
the contract, not from the kernel): synthetic trajectories, NaN poisoning of everything that must not be read, the log-probabilities,
determinism, collect end to end, graph capture, the error paths, the PPO example."""
import copy
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from pyflyt_amd import MLPPolicy, PyFlytAmdError, build_params
from pyflyt_amd import _lib as L
from pyflyt_amd.engine import BatchEngine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1000  # a ragged last wave (15 x 64 + 40)
U = 2.0 ** -24
MODES = ("next_step", "same_step", "off")


# ---------------------------------------------------------------------------------------------- the reference
def ref_gae(mode, gamma, lam, reward, terminated, truncated, values, final_values=None, episode_start=None):
    """float64, from the same float32 inputs (gamma and lambda as the float32 numbers the library receives)."""
    k, n = reward.shape
    g, l = float(np.float32(gamma)), float(np.float32(lam))
    r, v = reward.astype(np.float64), values.astype(np.float64)
    term, trunc = terminated.astype(bool), truncated.astype(bool)
    done = term | trunc
    valid = np.ones((k, n), dtype=bool)
    if mode == "next_step":  # step s only resets the lane iff the step before it finished the episode
        valid[0] = ~(episode_start.astype(bool) if episode_start is not None else np.zeros(n, dtype=bool))
        valid[1:] = ~done[:-1]
    adv, ret = np.zeros((k, n)), np.zeros((k, n))
    nxt = np.zeros(n)
    with np.errstate(invalid="ignore"):
        for s in reversed(range(k)):
            nv = v[s + 1]
            if mode == "same_step":
                nv = np.where(done[s], final_values[s].astype(np.float64), nv)
            delta = r[s] + g * np.where(term[s], 0.0, nv) - v[s]
            a = delta + g * l * np.where(done[s], 0.0, nxt)
            a = np.where(valid[s], a, 0.0)
            adv[s], ret[s] = a, np.where(valid[s], a + v[s], v[s])
            nxt = a
    return adv, ret, valid


def gae_bound(gamma, lam, k, reward, values, final_values=None, sel=None):
    """|adv - ref| <= 16 u M G^2 with u = 2^-24, M = max |r| + 2 max |V|, G = sum_{j < k} (gamma lambda)^j.
    Derivation: a valid step computes delta = fma(gamma, bootstrap, r) - V and adv = fma(gamma lambda, adv', delta): with the float32
    product gamma * lambda at most five roundings, each of a quantity bounded by M G (|delta| <= M, |adv| <= M G), so each step adds at
    most 5 u M G of error, and an error made at step s + j reaches step s scaled by (gamma lambda)^j: the sum over j is at most G times
    that, 5 u M G^2. returns = adv + V adds one more rounding of at most u M G. 16 leaves a factor of three over the count; a wrong
    mask or a wrong bootstrap is off by O(M), seven orders of magnitude more."""
    vmax = float(np.abs(values).max())
    if final_values is not None:
        vmax = max(vmax, float(np.abs(final_values[sel]).max()) if sel.any() else 0.0)
    M = float(np.abs(reward[np.isfinite(reward)]).max()) + 2.0 * vmax
    gl = float(np.float32(gamma)) * float(np.float32(lam))
    G = sum(gl ** j for j in range(k))
    return 16.0 * U * M * G * G


def synth(mode, k, n=N, seed=0):
    """Random rewards and values; flags with terminations, truncations, both at once, a lane finishing at s = 0, one at s = k - 1, one
    finishing twice (where k admits it), episode_start ones under NEXT_STEP. Under NEXT_STEP the step after a finished one is a reset
    step as pf_env_step writes it: reward 0, both flags 0."""
    rng = np.random.default_rng(1000 * k + seed)
    p = min(0.4, 3.0 / k)
    term = rng.random((k, n)) < p / 2
    trunc = rng.random((k, n)) < p / 2
    term[:, :4] = False
    trunc[:, :4] = False
    term[0, 0] = True           # lane 0 finishes at s = 0
    trunc[k - 1, 1] = True      # lane 1 at s = k - 1
    gap = 2 if mode == "next_step" else 1
    if k > gap:                 # lane 2 twice
        term[0, 2] = True
        trunc[gap, 2] = True
    reward = rng.normal(size=(k, n)).astype(np.float32) * 2.0
    values = rng.normal(size=(k + 1, n)).astype(np.float32) * 5.0
    final_values = rng.normal(size=(k, n)).astype(np.float32) * 5.0 if mode == "same_step" else None
    episode_start = None
    if mode == "next_step":
        episode_start = rng.random(n) < 0.1
        episode_start[:3] = False
        episode_start[3] = True
        prev = episode_start.copy()
        for s in range(k):
            term[s, prev] = False
            trunc[s, prev] = False
            reward[s, prev] = 0.0
            prev = term[s] | trunc[s]
    return dict(reward=reward, terminated=term, truncated=trunc, values=values, final_values=final_values, episode_start=episode_start)


def count_structure(mode, d):
    done = d["terminated"] | d["truncated"]
    k = done.shape[0]
    twice_possible = k > (2 if mode == "next_step" else 1)
    c = dict(terminations=int(d["terminated"].sum()), truncations=int(d["truncated"].sum()), at_first=int(done[0].sum()),
             at_last=int(done[k - 1].sum()), twice=int((done.sum(0) >= 2).sum()) if twice_possible else None,
             episode_start=int(d["episode_start"].sum()) if mode == "next_step" else None)
    return c


def engine(mode, n=N, task="hover", **kw):
    return BatchEngine(build_params("quadx", task, autoreset=mode, seed=3, **kw), n, device=DEV)


def to_dev(d):
    return {key: (None if v is None else torch.as_tensor(v, device=DEV).contiguous()) for key, v in d.items()}


def run_gae(eng, d, gamma, lam, **logp):
    t = to_dev(d)
    out = eng.gae(t["reward"], t["terminated"], t["truncated"], t["values"], gamma=gamma, lam=lam, final_values=t["final_values"],
                  episode_start=t["episode_start"], **logp)
    torch.cuda.synchronize()
    return [None if x is None else x.clone() for x in out]


# ---------------------------------------------------------------------------------------------- 1. synthetic trajectories
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [1, 7, 100])
@pytest.mark.parametrize("gamma, lam", [(0.99, 0.95), (1.0, 1.0), (0.9, 0.0)])
def test_synthetic_trajectories(mode, k, gamma, lam):
    d = synth(mode, k)
    c = count_structure(mode, d)
    print(mode, k, c)
    assert all(v is None or v > 0 for v in c.values()), c  # (not vacuous: every kind of event is in the case)
    eng = engine(mode)
    adv, ret, logp, valid = run_gae(eng, d, gamma, lam)
    assert logp is None
    radv, rret, rvalid = ref_gae(mode, gamma, lam, **d)
    valid = valid.cpu().numpy()
    assert valid.dtype == np.bool_ and np.array_equal(valid, rvalid)
    if mode == "next_step":
        assert int((~rvalid).sum()) > 0
    else:
        assert rvalid.all()
    adv, ret = adv.cpu().numpy(), ret.cpu().numpy()
    done = d["terminated"] | d["truncated"]
    bound = gae_bound(gamma, lam, k, d["reward"], d["values"], d["final_values"], done)
    ea, er = np.abs(adv - radv).max(), np.abs(ret - rret).max()
    print(f"{mode} k {k} gamma {gamma} lambda {lam}: advantages off by {ea:.3e}, returns by {er:.3e}, bound {bound:.3e}")
    assert ea <= bound and er <= bound
    inv = ~rvalid
    assert np.array_equal(adv[inv].view(np.uint32), np.zeros(int(inv.sum()), dtype=np.uint32))  # +0.0, bit for bit
    assert np.array_equal(ret[inv].view(np.uint32), d["values"][:-1][inv].view(np.uint32))
    eng.close()


# ---------------------------------------------------------------------------------------------- 2. poisoning
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [7, 100])
def test_poisoned_inputs_reach_no_valid_output(mode, k):
    """NaN in every final_values row of a lane that did not finish, and in the reward of every invalid step: the outputs of the valid
    steps are finite and the same bits as without the poison (a mask applied by multiplication would turn them into NaN)."""
    d = synth(mode, k, seed=1)
    eng = engine(mode)
    clean = run_gae(eng, d, 0.99, 0.95)
    _, _, rvalid = ref_gae(mode, 0.99, 0.95, **d)
    p = {key: (None if v is None else v.copy()) for key, v in d.items()}
    done = d["terminated"] | d["truncated"]
    poisoned = 0
    if mode == "same_step":
        p["final_values"][~done] = np.nan
        poisoned += int((~done).sum())
    if mode == "next_step":
        p["reward"][~rvalid] = np.nan
        poisoned += int((~rvalid).sum())
    if mode != "off":
        assert poisoned > 0
    dirty = run_gae(eng, p, 0.99, 0.95)
    for name, a, b in zip(("advantages", "returns"), clean[:2], dirty[:2]):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert np.isfinite(b[rvalid]).all(), name
        assert np.array_equal(a[rvalid].view(np.uint32), b[rvalid].view(np.uint32)), name
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name  # (and the invalid steps' constants as well)
    assert torch.equal(clean[3], dirty[3])
    eng.close()


# ---------------------------------------------------------------------------------------------- 3. log-probabilities
def logp_bound(log_std, A=4):
    """Per component -1/2 z^2 - log_std - 1/2 log(2 pi) with z = (a - mean) exp(-log_std), |z| <= 4.86 (the header's guarantee for
    the actions pf_rollout_policy samples). z carries about three roundings (the difference, the exponential, the product), so z^2 is
    off by at most 8 u relatively with its own product: 1/2 4.86^2 8 u; the two subtractions and the running sum add at most
    4 u (|log_std| + 1). Over A components: A (1/2 4.86^2 8 u + 4 u (|log_std| + 1))."""
    return A * (0.5 * 4.86 ** 2 * 8 * U + 4 * U * (float(np.abs(log_std).max()) + 1.0))


@pytest.mark.parametrize("mode", ["next_step", "same_step"])
def test_log_probabilities(mode):
    k = 40
    d = synth(mode, k, seed=2)
    rng = np.random.default_rng(5)
    log_std = np.array([-1.0, -0.5, 0.0, 0.3], dtype=np.float32)
    mean = rng.normal(size=(k, N, 4)).astype(np.float32)
    eps = np.clip(rng.normal(size=(k, N, 4)), -4.86, 4.86).astype(np.float32)
    eps[0, 0] = (4.86, -4.86, 0.0, 4.86)
    actions = (mean + np.exp(log_std) * eps).astype(np.float32)
    eng = engine(mode)
    t = to_dev(dict(actions=actions, mean=mean, log_std=log_std))
    _, _, logp, _ = run_gae(eng, d, 0.99, 0.95, **t)
    ref = torch.distributions.Normal(t["mean"].double(), t["log_std"].double().exp()).log_prob(t["actions"].double()).sum(-1)
    z = ((t["actions"].double() - t["mean"].double()) / t["log_std"].double().exp()).abs().max().item()
    err = (logp.double() - ref).abs().max().item()
    bound = logp_bound(log_std)
    print(f"{mode}: log-probabilities off by {err:.3e}, bound {bound:.3e}, largest |z| {z:.4f}")
    assert z <= 4.86 * (1 + 1e-6)
    assert logp.shape == (k, N) and err <= bound
    eng.close()


# ---------------------------------------------------------------------------------------------- 4. determinism
@pytest.mark.parametrize("mode", MODES)
def test_bits_do_not_depend_on_the_call_or_the_lane_count(mode):
    k, shift = 100, 37
    d = synth(mode, k, seed=3)
    rng = np.random.default_rng(9)
    lp = dict(actions=rng.normal(size=(k, N, 4)).astype(np.float32), mean=rng.normal(size=(k, N, 4)).astype(np.float32),
              log_std=np.array([-0.3, 0.1, -1.2, 0.0], dtype=np.float32))
    eng = engine(mode)
    a = run_gae(eng, d, 0.99, 0.95, **to_dev(lp))
    b = run_gae(eng, d, 0.99, 0.95, **to_dev(lp))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # the same lanes at another place (another wave, another position in it) of a context twice as large
    big = synth(mode, k, n=2 * N, seed=4)
    lpb = dict(actions=rng.normal(size=(k, 2 * N, 4)).astype(np.float32), mean=rng.normal(size=(k, 2 * N, 4)).astype(np.float32), log_std=lp["log_std"])
    for key, v in d.items():
        if v is not None:
            big[key][..., shift:shift + N] = v
    for key in ("actions", "mean"):
        lpb[key][:, shift:shift + N] = lp[key]
    eng2 = engine(mode, n=2 * N)
    c = run_gae(eng2, big, 0.99, 0.95, **to_dev(lpb))
    for x, y in zip(a, c):
        assert torch.equal(x, y[:, shift:shift + N])
    eng.close(); eng2.close()


# ---------------------------------------------------------------------------------------------- 5. end to end
def make_env(task, mode, n=N, seed=11):
    from pyflyt_amd.gym_envs import make_vec

    env_id = "PyFlyt/QuadX-Hover-v4" if task == "hover" else "PyFlyt/QuadX-Waypoints-v4"
    return make_vec(env_id, n, seed=seed, autoreset_mode=mode, max_duration_seconds=1.0)


def make_nets(obs_dim):
    g = torch.Generator().manual_seed(5)
    sizes = [obs_dim, 64, 64, 4]
    ls = [((torch.randn(o, i, generator=g) * 1.2 / math.sqrt(i)).to(DEV).contiguous(), (torch.randn(o, generator=g) * 0.1).to(DEV))
          for i, o in zip(sizes[:-1], sizes[1:])]
    pol = MLPPolicy(ls, log_std=torch.zeros(4, device=DEV))  # std 1: the drones tumble; the dome, the floor and the 1 s limit end episodes
    torch.manual_seed(7)
    nn = torch.nn
    vnet = nn.Sequential(nn.Linear(obs_dim, 32), nn.Tanh(), nn.Linear(32, 1)).to(DEV)
    return pol, vnet


@pytest.mark.parametrize("task", ["hover", "waypoints"])
@pytest.mark.parametrize("mode", ["next_step", "same_step"])
def test_collect_end_to_end(task, mode):
    k, gamma, lam = 96, 0.99, 0.95
    env = make_env(task, mode)
    returned = env.reset()[0]
    obs0 = env.engine.obs.clone()  # (the flat rows the policy reads; Hover returns exactly them, Waypoints a dict of views of them)
    assert torch.equal(returned, obs0) if torch.is_tensor(returned) else torch.equal(returned["attitude"], obs0[:, :returned["attitude"].shape[1]])
    pol, vnet = make_nets(env.engine.obs_dim)
    seen = []

    def value_fn(o):
        assert not torch.is_grad_enabled() and o.dtype == torch.float32 and o.dim() == 2
        seen.append(vnet(o))
        return seen[-1]

    es = ((env.engine.flags() & 3) != 0).cpu().numpy()
    b = env.collect(pol, value_fn, k, gamma=gamma, lam=lam)
    torch.cuda.synchronize()
    assert len(seen) == (2 if mode == "same_step" else 1) and seen[0].shape[0] == (k + 1) * N
    term, trunc = b["terminated"].cpu().numpy(), b["truncated"].cpu().numpy()
    n_reset = int((~b["valid"]).sum())
    print(f"{task} {mode}: {int(term.sum())} terminations, {int(trunc.sum())} truncations, {n_reset} reset steps")
    assert term.sum() > 0 and trunc.sum() > 0
    assert (n_reset > 0) if mode == "next_step" else (n_reset == 0)
    assert not es.any()  # (after reset() no lane waits for its reset)
    assert torch.equal(b["obs"][0], obs0)
    assert b["obs"].shape == (k, N, env.engine.obs_dim) and b["values"].shape == (k, N) and b["last_value"].shape == (N,)
    values = torch.cat([b["values"], b["last_value"][None]], 0)
    assert torch.equal(values.reshape(-1), seen[0].reshape(-1))
    # the value net in float64 agrees with what collect() used (a wiring check: the right rows went through value_fn) ...
    vnet64 = copy.deepcopy(vnet).double()
    v64 = vnet64(b["obs"].double()).squeeze(-1)
    assert (v64 - b["values"].double()).abs().max().item() < 1e-2  # (float32 GEMM on tumbling drones' observations; a wrong row is off by O(1))
    # ... and the reference takes the float32 values collect() returns
    fv = seen[1].reshape(k, N).cpu().numpy() if mode == "same_step" else None
    radv, rret, rvalid = ref_gae(mode, gamma, lam, b["reward"].cpu().numpy(), term, trunc, values.cpu().numpy(), fv, es if mode == "next_step" else None)
    assert np.array_equal(b["valid"].cpu().numpy(), rvalid)
    bound = gae_bound(gamma, lam, k, b["reward"].cpu().numpy(), values.cpu().numpy(), fv, term | trunc)
    ea = np.abs(b["advantages"].cpu().numpy() - radv).max()
    er = np.abs(b["returns"].cpu().numpy() - rret).max()
    ref_lp = torch.distributions.Normal(b["mean"].double(), pol.log_std.double().exp()).log_prob(b["actions"].double()).sum(-1)
    el = (b["logp"].double() - ref_lp).abs().max().item()
    print(f"{task} {mode}: advantages off by {ea:.3e}, returns by {er:.3e} (bound {bound:.3e}); log-probabilities by {el:.3e} (bound {logp_bound(np.zeros(4)):.3e})")
    assert ea <= bound and er <= bound and el <= logp_bound(np.zeros(4))
    # a second call continues: its first policy input is the first call's last observation, and lanes that finished in the last step
    # start with a reset step
    last_value, last_done = b["last_value"].clone(), (b["terminated"][-1] | b["truncated"][-1]).clone()
    b2 = env.collect(pol, value_fn, k, gamma=gamma, lam=lam)
    assert (vnet64(b2["obs"][0].double()).squeeze(-1) - last_value.double()).abs().max().item() < 1e-2  # (last_value IS the value of that row)
    if mode == "next_step":
        assert int(last_done.sum()) > 0 and torch.equal(~b2["valid"][0], last_done)
    # views, not copies: the engine's rollout for a learner hands out the buffers collect() returns views of (the same tensors at
    # every call with the same k): the policy input of step s + 1 IS the row the launch writes as step s's next observation
    t = env.engine.collect_rollout(pol, k, step_index0=env._policy_step)
    assert t["obs_all"].data_ptr() == b2["obs"].data_ptr() == b["obs"].data_ptr() and t["obs_all"].shape[0] == k + 1
    for s in (0, 1, k - 2):
        assert b2["obs"][s + 1].data_ptr() == t["obs"][s].data_ptr()
    env.close()


@pytest.mark.parametrize("mode", ["next_step", "same_step"])
def test_two_collects_are_one_rollout(mode):
    k = 96
    e1, e2 = make_env("hover", mode), make_env("hover", mode)
    e1.reset(); e2.reset()
    pol, vnet = make_nets(e1.engine.obs_dim)
    halves = []
    for _ in range(2):
        b = e1.collect(pol, vnet, k // 2)
        halves.append({key: b[key].clone() for key in ("obs", "actions", "reward", "terminated", "truncated", "mean")})
    full = e2.rollout(pol, k, store_mean=True)
    for key, f in zip(("obs", "reward", "terminated", "truncated", "actions", "mean"), full):
        got = torch.cat([halves[0][key], halves[1][key]], 0)
        if key == "obs":  # (collect's obs are the policy's INPUTS, rollout's the next observations: the same rows, shifted by one step)
            got, f = got[1:], f[:-1]
        assert torch.equal(got, f), key
    assert torch.equal(e1.engine.state, e2.engine.state)
    assert e1._policy_step == e2._policy_step == k
    e1.close(); e2.close()


def test_collect_refuses_what_the_rollout_refuses():
    from pyflyt_amd.gym_envs import make_vec

    env = make_vec("PyFlyt/QuadX-Hover-v4", 64, autoreset_mode="disabled")
    env.reset()
    pol, vnet = make_nets(env.engine.obs_dim)
    with pytest.raises(PyFlytAmdError) as e:
        env.collect(pol, vnet, 4)
    assert e.value.code == L.ERR_UNSUPPORTED and "pf_rollout_policy: needs an auto-reset mode" in str(e.value)
    env.close()


# ---------------------------------------------------------------------------------------------- 6. graph capture
def test_gae_is_capturable():
    mode, k = "same_step", 20
    d = synth(mode, k, seed=6)
    rng = np.random.default_rng(2)
    lp = to_dev(dict(actions=rng.normal(size=(k, N, 4)).astype(np.float32), mean=rng.normal(size=(k, N, 4)).astype(np.float32),
                     log_std=np.zeros(4, dtype=np.float32)))
    t = to_dev(d)
    eng = engine(mode)

    def call():
        return eng.gae(t["reward"], t["terminated"], t["truncated"], t["values"], gamma=0.99, lam=0.95, final_values=t["final_values"], **lp)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = [x.clone() for x in out]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    for x in out:
        x.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(out, eager):
        assert torch.equal(x, y)
    assert float(eager[0].abs().sum()) > 0
    eng.close()


# ---------------------------------------------------------------------------------------------- 7. error paths
def test_error_paths_name_the_argument():
    k = 4
    for mode in MODES:
        eng = engine(mode, n=64)
        f32 = dict(dtype=torch.float32, device=DEV)
        buf = dict(reward=torch.zeros(k, 64, **f32), terminated=torch.zeros(k, 64, dtype=torch.bool, device=DEV),
                   truncated=torch.zeros(k, 64, dtype=torch.bool, device=DEV), values=torch.zeros(k + 1, 64, **f32),
                   advantages=torch.zeros(k, 64, **f32), returns=torch.zeros(k, 64, **f32), final_values=torch.zeros(k, 64, **f32),
                   episode_start=torch.zeros(64, dtype=torch.bool, device=DEV), actions=torch.zeros(k, 64, 4, **f32),
                   mean=torch.zeros(k, 64, 4, **f32), log_std=torch.zeros(4, **f32), logp_out=torch.zeros(k, 64, **f32))

        def block(**change):
            a = L.PfGae()
            a.gamma, vals = 0.99, dict(buf)
            setattr(a, "lambda", 0.95)
            if mode != "same_step":
                vals["final_values"] = None
            if mode != "next_step":
                vals["episode_start"] = None
            for key, v in {**vals, **change}.items():
                setattr(a, key, v if isinstance(v, float) or v is None else v.data_ptr())
            return a

        def refused(fragment, steps=k, **change):
            a = block(**change)
            rc = eng.lib.pf_gae(eng._ctx, C.byref(a), steps, eng._stream())
            msg = eng.lib.pf_last_error(eng._ctx).decode()
            assert rc == L.ERR_ARG and fragment in msg, (rc, msg)

        assert eng.lib.pf_gae(eng._ctx, C.byref(block()), k, eng._stream()) == 0  # (the unchanged block is accepted)
        refused("k_steps", steps=0)
        for name in ("reward", "terminated", "truncated", "values", "advantages", "returns"):
            refused(name, **{name: None})
        refused("gamma", gamma=1.5)
        refused("gamma", gamma=float("nan"))
        refused("lambda", **{"lambda": -0.25})
        refused("lambda", **{"lambda": float("inf")})
        if mode == "same_step":
            refused("final_values is required", final_values=None)
        else:
            refused("final_values must be NULL", final_values=buf["final_values"])
        if mode != "next_step":
            refused("episode_start", episode_start=buf["episode_start"])
        for name in ("actions", "mean", "log_std", "logp_out"):
            refused("actions, mean, log_std and logp_out", **{name: None})
        torch.cuda.synchronize()
        eng.close()
    aviary = BatchEngine(build_params("quadx", "none"), 64, device=DEV)  # (no env task: there is no trajectory to post-process)
    rc = aviary.lib.pf_gae(aviary._ctx, C.byref(L.PfGae()), 4, aviary._stream())
    assert rc == L.ERR_UNSUPPORTED and "env task" in aviary.lib.pf_last_error(aviary._ctx).decode()
    aviary.close()


# ---------------------------------------------------------------------------------------------- 8. the example
def test_example_06_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "06_ppo_hover.py"), "4096", "2"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rewards = [float(x) for x in re.findall(r"mean reward per valid step ([-+0-9.eE]+|nan|inf)", out.stdout)]
    assert len(rewards) == 2 and all(math.isfinite(r) for r in rewards), out.stdout
    moved = re.search(r"parameters moved by ([-+0-9.eE]+|nan|inf)", out.stdout)
    assert moved and math.isfinite(float(moved.group(1))) and float(moved.group(1)) > 0.0, out.stdout

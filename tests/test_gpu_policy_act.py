"""pf_policy_act on the device: bitwise against the fused rollout launch where both exist, against an fp64 forward where only it
exists, the documented draw for six- and seven-wide heads, the stepwise rollout / collect on every vector env, refusals, graph
capture, full size, the example."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pyflyt_amd import MLPPolicy, PyFlytAmdError, build_params
from pyflyt_amd import _lib as L
from pyflyt_amd.engine import BatchEngine
from test_gpu_gae import logp_bound
from test_gpu_policy_rollout import CASES, bm16_np, engine as quad_engine, philox_np, run_policy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, OFFSET = 1000, 70_001  # 15 tiles of 64 rows plus 40 rows; a lane offset != 0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETS = [((64, 64), "tanh"), ((33, 64), "relu"), ((1,), "tanh"), ((64, 1), "tanh")]


def net(obs_dim, act_dim, hidden=(64, 64), activation="tanh", log_std=-0.2, seed=5, scale=0.4):
    """test_gpu_policy_rollout.policy with the action width as an argument."""
    g = torch.Generator().manual_seed(seed)
    sizes = [obs_dim, *hidden, act_dim]
    ls = [((torch.randn(o, i, generator=g) * scale / math.sqrt(i) * 3.0).to(DEV).contiguous(), (torch.randn(o, generator=g) * 0.1).to(DEV))
          for i, o in zip(sizes[:-1], sizes[1:])]
    return MLPPolicy(ls, activation=activation, log_std=None if log_std is None else torch.full((act_dim,), float(log_std), device=DEV))


def value_net(obs_dim):
    torch.manual_seed(7)
    nn = torch.nn
    return nn.Sequential(nn.Linear(obs_dim, 32), nn.Tanh(), nn.Linear(32, 1)).to(DEV)


def other_engine(kind, n, **kw):
    """The contexts pf_rollout_policy refuses."""
    if kind == "fixedwing":
        P = build_params("fixedwing", "waypoints", seed=11, **kw)
    elif kind in ("rocket_quat", "rocket_euler"):
        P = build_params("rocket", "rocket_landing", seed=11, angle_representation="quaternion" if kind == "rocket_quat" else "euler", **kw)
    elif kind == "dogfight":
        P = build_params("fixedwing", "dogfight", seed=11, autoreset="off", angle_representation="euler", vehicle_options=dict(drone_model="acrowing"),
                         dogfight=dict(team_size=4, assisted_flight=False), **kw)
    else:
        P = build_params("quadx", "hover", seed=11, flight_mode=6, **kw)
    return BatchEngine(P, n, device=DEV, lane_offset=OFFSET)


# ---------------------------------------------------------------------------------------------- 1. bitwise against the fused launch
@pytest.mark.parametrize("task, noise, autoreset", CASES)
@pytest.mark.parametrize("hidden, activation", NETS)
def test_bitwise_against_the_fused_launch(task, noise, autoreset, hidden, activation):
    """k x (policy_act(step0 + s) on the current observation, env_step) against rollout_policy(k, step0): every bit. The time limit is
    10 steps (0.25 s at 40 Hz; a Hover episode is truncated in its 12th step): every lane ends an episode and is reset inside the 24
    steps, twice except on Hover under NEXT_STEP, where the second end would be step 25 (measured: ends at steps 11 and 23 under
    SAME_STEP, 11 under NEXT_STEP; Waypoints 8 and 17 / 18)."""
    k, step0 = 24, 50
    ea, eb = (quad_engine(task, noise, autoreset, max_duration_seconds=0.25) for _ in range(2))
    ea.env_reset(); eb.env_reset()
    pol = net(ea.obs_dim, 4, hidden, activation, log_std=0.0)
    a = run_policy(ea, pol, k=k, step0=step0)
    f32 = dict(dtype=torch.float32, device=DEV)
    b = dict(actions=torch.empty(k, N, 4, **f32), mean=torch.empty(k, N, 4, **f32), obs=torch.empty(k, N, eb.obs_dim, **f32),
             reward=torch.empty(k, N, **f32), terminated=torch.empty(k, N, dtype=torch.bool, device=DEV),
             truncated=torch.empty(k, N, dtype=torch.bool, device=DEV))
    if eb.final_obs is not None:
        b["final_obs"], b["final_info"] = torch.zeros(k, N, eb.obs_dim, **f32), torch.zeros(k, N, 2, dtype=torch.int32, device=DEV)
    for s in range(k):
        eb.policy_act(pol, step_index=step0 + s, out=b["actions"][s], mean_out=b["mean"][s])
        o, r, te, tr = eb.env_step(b["actions"][s])
        b["obs"][s], b["reward"][s], b["terminated"][s], b["truncated"][s] = o, r, te, tr
        if eb.final_obs is not None:
            b["final_obs"][s], b["final_info"][s] = eb.final_obs, eb.final_info
    done = a["terminated"] | a["truncated"]
    ends = done.sum(0)
    print(f"{task} {noise} {autoreset} {hidden} {activation}: episode ends per lane {int(ends.min())} .. {int(ends.max())}, lane 0 at steps "
          f"{done[:, 0].nonzero().flatten().tolist()}")
    assert int(ends.min()) >= 1  # (every lane crosses an episode end and its auto-reset inside the run)
    for key in ("actions", "mean", "obs", "reward", "terminated", "truncated"):
        assert torch.equal(a[key], b[key]), key
    assert torch.equal(a["state"], eb.state)
    if "final_obs" in b:
        for key in ("final_obs", "final_info"):
            assert torch.equal(a[key][done], b[key][done]), key
    # ... and the engine's own stepwise rollout is that loop
    ec = quad_engine(task, noise, autoreset, max_duration_seconds=0.25)
    ec.env_reset()
    out = ec.rollout_policy_steps(pol, k, step_index0=step0, store_mean=True)
    for key, v in zip(("obs", "reward", "terminated", "truncated", "actions", "mean"), out):
        assert torch.equal(a[key], v), key
    assert torch.equal(a["state"], ec.state)
    if "final_obs" in b:
        for key in ("final_obs", "final_info"):
            assert torch.equal(a[key][done], ec._traj[key][done]), key


# ---------------------------------------------------------------------------------------------- 2. against fp64
def mean_error_ratio(pol, obs, mean):
    """(largest deviation of `mean` from the fp64 forward on `obs`, e32 = that of torch's own float32 forward)."""
    ref = pol.forward_reference(obs, dtype=torch.float64)
    e32 = (pol.forward_reference(obs, dtype=torch.float32).double() - ref).abs().max().item()
    return (mean.double() - ref).abs().max().item(), e32


@pytest.mark.parametrize("kind, n", [(kind, n) for kind in ("fixedwing", "rocket_quat", "rocket_euler", "dogfight", "hover_mode6") for n in (1000, 1, 64)
                                     if not (kind == "dogfight" and n == 1)])
def test_against_fp64_where_no_fused_path_exists(kind, n):
    """Bound: pf_rollout_policy's own, 8 x e32 (tests/test_gpu_policy_rollout.py: the same precision, another summation order,
    another tanh)."""
    eng = other_engine(kind, n)
    D, A = eng.obs_dim, eng.action_dim
    assert (D, A) == {"fixedwing": (35, 4), "rocket_quat": (30, 7), "rocket_euler": (29, 7), "dogfight": (123, 6), "hover_mode6": (21, 4)}[kind]
    obs = eng.env_reset().clone()
    for hidden, activation in (((64, 64), "tanh"), ((33,), "relu")):
        pol = net(D, A, hidden, activation)
        mean = torch.full((n, A), float("nan"), device=DEV)
        actions, m = eng.policy_act(pol, step_index=3, mean_out=mean)
        assert m is mean and actions.shape == (n, A)
        err, e32 = mean_error_ratio(pol, obs, mean)
        print(f"{kind} n {n} {hidden} {activation}: D {D}, A {A}, kernel deviation {err:.3e}, torch float32 deviation e32 {e32:.3e}, ratio {err / e32:.2f}")
        assert err <= 8.0 * e32
        assert torch.isfinite(actions).all() and not torch.equal(actions, mean)
        det = MLPPolicy(pol.layers, activation=activation, log_std=None)
        mean2 = torch.empty_like(mean)
        a2 = eng.policy_act(det, step_index=3, obs=obs, mean_out=mean2)[0]
        assert torch.equal(a2, mean2) and torch.equal(mean2, mean)  # deterministic head: the action IS the mean
    assert torch.equal(eng.obs, obs)  # (the call reads its rows)
    eng.close()


# ---------------------------------------------------------------------------------------------- 3. the draw
@pytest.mark.parametrize("kind", ["rocket_quat", "dogfight"])
def test_the_draw_is_the_documented_one(kind):
    """Philox (seed, global lane, step_index, 0), stream 4; eps_c = normal c of the call's eight, c < A (A = 7 and 6)."""
    eng = other_engine(kind, N)
    eng.env_reset()
    A, ls, step = eng.action_dim, -0.5, 1234
    pol = net(eng.obs_dim, A, log_std=ls)
    mean = torch.empty(N, A, device=DEV)
    actions = eng.policy_act(pol, step_index=step, mean_out=mean)[0]
    eps = ((actions.double() - mean.double()) / math.exp(ls)).cpu().numpy()
    seed = int(eng.params.seed)
    lanes = (OFFSET + np.arange(N)).astype(np.uint32)
    w = philox_np(seed & 0xFFFFFFFF, seed >> 32, lanes, np.uint32(step), np.uint32(0), np.uint32(4))
    want = np.stack([z for word in w for z in bm16_np(word)], -1)[:, :A]
    assert np.abs(eps - want).max() < 1e-3  # (v_log / v_sin / v_cos against libm, and the read-back rounding: test_gpu_policy_rollout.py)
    again = eng.policy_act(pol, step_index=step)
    other = eng.policy_act(pol, step_index=step + 1)
    assert torch.equal(again, actions) and not torch.equal(other, actions)
    eng.close()


# ---------------------------------------------------------------------------------------------- 4. stepwise collect == fused collect
@pytest.mark.parametrize("mode", ["next_step", "same_step"])
def test_stepwise_collect_equals_fused_collect_on_hover(mode):
    from pyflyt_amd.gym_envs import make_vec

    k = 48
    envs = [make_vec("PyFlyt/QuadX-Hover-v4", N, seed=11, autoreset_mode=mode, max_duration_seconds=1.0, lane_offset=OFFSET) for _ in range(2)]
    pol, vnet = net(21, 4, log_std=0.0), value_net(21)
    for env in envs:
        env.reset()
    for call in range(2):
        ba = envs[0].collect(pol, vnet, k, stats=True, fused=False)
        bb = envs[1].collect(pol, vnet, k, stats=True)
        assert set(ba) == set(bb)
        for key in ba:
            if torch.is_tensor(ba[key]):
                assert torch.equal(ba[key], bb[key]), (call, key)
            else:
                assert key == "infos" or (ba[key] is None and bb[key] is None), key
        assert int((ba["terminated"] | ba["truncated"]).sum()) >= N
        assert torch.equal(envs[0].engine.state, envs[1].engine.state)
        assert envs[0]._policy_step == envs[1]._policy_step == k * (call + 1)
        assert torch.equal(envs[0].engine.obs_moments, envs[1].engine.obs_moments) and torch.equal(envs[0].engine.ret_moments, envs[1].engine.ret_moments)
    for env in envs:
        env.close()


# ---------------------------------------------------------------------------------------------- 5. the other vector envs
def other_env(kind, mode, n=N, **kw):
    from pyflyt_amd.gym_envs import make_vec
    from pyflyt_amd.gym_envs.vector_envs import RocketLandingVecEnv

    kw = dict(dict(seed=11, autoreset_mode=mode, max_duration_seconds=1.0, lane_offset=OFFSET), **kw)
    return make_vec("PyFlyt/Fixedwing-Waypoints-v4", n, **kw) if kind == "fixedwing" else RocketLandingVecEnv(n, **kw)


def collect_and_replay(kind, mode, n, k, offset=OFFSET):
    """env.collect with the default `fused`, then the returned actions through env.step on a second env: row for row the same bits."""
    env, env2 = (other_env(kind, mode, n=n, lane_offset=offset) for _ in range(2))
    env.reset(); env2.reset()
    eng = env.engine
    pol, vnet = net(eng.obs_dim, eng.action_dim, log_std=0.0), value_net(eng.obs_dim)
    obs0 = eng.obs.clone()
    b = env.collect(pol, vnet, k)
    assert torch.equal(b["obs"][0], obs0)
    nxt = eng._ctraj["obs"]  # (obs_all[1:]: what the env wrote at each step)
    for s in range(k):
        env2.step(b["actions"][s])
        e2 = env2.engine
        assert torch.equal(e2.obs, nxt[s]) and torch.equal(e2.reward, b["reward"][s]), s
        assert torch.equal(e2.terminated, b["terminated"][s]) and torch.equal(e2.truncated, b["truncated"][s]), s
        if s + 1 < k:
            assert nxt[s].data_ptr() == b["obs"][s + 1].data_ptr()
    assert torch.equal(env2.engine.state, eng.state)
    return env, env2, pol, b


@pytest.mark.parametrize("kind", ["fixedwing", "rocket"])
@pytest.mark.parametrize("mode", ["next_step", "same_step"])
def test_collect_on_the_other_vector_envs(kind, mode):
    k = 48
    env, env2, pol, b = collect_and_replay(kind, mode, N, k)
    A = env.engine.action_dim
    assert b["actions"].shape == b["mean"].shape == (k, N, A)
    err, e32 = mean_error_ratio(pol, b["obs"], b["mean"])
    print(f"{kind} {mode}: means off by {err:.3e}, torch float32 by {e32:.3e}, ratio {err / e32:.2f}")
    assert err <= 8.0 * e32
    done = b["terminated"] | b["truncated"]
    assert int(done.sum()) >= N  # (the 1 s limit)
    want_valid = torch.ones_like(done)
    if mode == "next_step":
        want_valid[1:] = ~done[:-1]
    assert torch.equal(b["valid"], want_valid)
    ref_lp = torch.distributions.Normal(b["mean"].double(), pol.log_std.double().exp()).log_prob(b["actions"].double()).sum(-1)
    el = (b["logp"].double() - ref_lp).abs().max().item()
    print(f"{kind} {mode}: log-probabilities off by {el:.3e} (bound {logp_bound(np.zeros(A), A):.3e})")
    assert el <= logp_bound(np.zeros(A), A)
    env.close(); env2.close()


# ---------------------------------------------------------------------------------------------- 6. refusals and arguments
def _raises(code, fragment, fn):
    with pytest.raises(PyFlytAmdError) as e:
        fn()
    assert e.value.code == code and fragment in str(e.value), str(e.value)


def test_refusals_and_arguments():
    from pyflyt_amd.gym_envs import make_vec

    eng = other_engine("fixedwing", 64)
    eng.env_reset()
    pol = net(eng.obs_dim, 4, hidden=(8, 8))
    out = torch.zeros(64, 4, device=DEV)

    def raw(edit=None, policy=True, actions=True, e=eng):
        q = pol.fill(L.PfPolicy(), e) if e is eng else net(e.obs_dim, 4, hidden=(8, 8)).fill(L.PfPolicy(), e)
        q.obs0 = e.obs.data_ptr()
        if edit:
            edit(q)
        return lambda: L.check(e.lib.pf_policy_act(e._ctx, C.byref(q) if policy else None, out.data_ptr() if actions else None, 0, e._stream()), e._ctx)

    def setter(name, value, index=None):
        def edit(q):
            if index is None:
                setattr(q, name, value)
            else:
                getattr(q, name)[index] = value
        return edit

    A, U = L.ERR_ARG, L.ERR_UNSUPPORTED
    _raises(A, "policy is required", raw(policy=False))
    _raises(A, "obs0", raw(setter("obs0", None)))
    _raises(A, "actions_out is required", raw(actions=False))
    _raises(A, "every layer needs w and b", raw(setter("w", None, 1)))
    _raises(A, "every layer needs w and b", raw(setter("b", None, 2)))
    _raises(A, "n_layers must be 2 or 3", raw(setter("n_layers", 4)))
    _raises(A, "n_layers must be 2 or 3", raw(setter("n_layers", 1)))
    _raises(A, "hidden widths must be >= 1", raw(setter("width", 0, 1)))
    _raises(A, "activation must be", raw(setter("activation", 7)))
    _raises(U, "PF_POLICY_MAX_HIDDEN", raw(setter("width", 65, 0)))
    aviary = BatchEngine(build_params("quadx", "none"), 64, device=DEV)
    _raises(U, "needs a context with an env task", raw(e=aviary))
    raw()()  # (the unedited block runs)
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="obs must be a contiguous float32 tensor"):
        eng.policy_act(pol, obs=torch.zeros(64, eng.obs_dim + 1, device=DEV))
    with pytest.raises(ValueError, match="out must be"):
        eng.policy_act(pol, out=torch.zeros(64, 5, device=DEV))
    with pytest.raises(ValueError, match="the env's action width is 4"):
        eng.policy_act(net(eng.obs_dim, 7))
    # the facade
    vnet = value_net(eng.obs_dim)
    env = make_vec("PyFlyt/Fixedwing-Waypoints-v4", 64, autoreset_mode="disabled")
    env.reset()
    state = env.engine.state.clone()
    with pytest.raises(ValueError, match="auto-reset"):
        env.collect(pol, vnet, 4)
    with pytest.raises(ValueError, match="auto-reset"):
        env.rollout(pol, 4)
    assert torch.equal(env.engine.state, state)  # (refused before any launch)
    env.close()
    inject = BatchEngine(build_params("fixedwing", "waypoints", noise="inject"), 64, device=DEV)
    for call in (lambda: inject.rollout_policy_steps(pol, 4), lambda: inject.collect_rollout(pol, 4)):
        with pytest.raises(ValueError, match="PF_NOISE_INJECT"):
            call()
    hover = make_vec("PyFlyt/QuadX-Hover-v4", 64, autoreset_mode="disabled")
    hover.reset()
    with pytest.raises(ValueError, match="auto-reset"):
        hover.rollout(net(21, 4), 4, fused=False)
    hover.close()
    env = make_vec("PyFlyt/Fixedwing-Waypoints-v4", 64)
    env.reset()
    for call in (lambda: env.rollout(pol, 4, fused="yes"), lambda: env.collect(pol, vnet, 4, fused="yes"), lambda: env.collect(pol, vnet, 4, fused=1)):
        with pytest.raises(ValueError, match="fused must be None, True or False"):
            call()
    _raises(U, "pf_rollout_policy: QuadX-Hover and QuadX-Waypoints only", lambda: env.rollout(pol, 4, fused=True))
    _raises(U, "pf_rollout_policy: QuadX-Hover and QuadX-Waypoints only", lambda: env.collect(pol, vnet, 4, fused=True))
    env.close()


# ---------------------------------------------------------------------------------------------- 7. graph capture
def test_act_and_step_are_capturable():
    pairs = 4
    eng = other_engine("fixedwing", N)
    eng.env_reset()
    pol = net(eng.obs_dim, 4, log_std=0.0)
    f32 = dict(dtype=torch.float32, device=DEV)
    acts, means, rec = torch.zeros(pairs, N, 4, **f32), torch.zeros(pairs, N, 4, **f32), torch.zeros(pairs, N, eng.obs_dim, **f32)

    def run():
        for s in range(pairs):
            eng.policy_act(pol, step_index=10 + s, obs=eng.obs, out=acts[s], mean_out=means[s])
            eng.env_step(acts[s])
            rec[s].copy_(eng.obs)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eng.policy_act(pol, step_index=9, obs=eng.obs, out=acts[0])  # warm-up
        eng.env_step(acts[0])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    state0, obs0 = eng.state.clone(), eng.obs.clone()
    run()
    torch.cuda.synchronize()
    eager = [x.clone() for x in (acts, means, rec, eng.state, eng.reward, eng.terminated, eng.truncated)]
    eng.state.copy_(state0); eng.obs.copy_(obs0)
    for x in (acts, means, rec):
        x.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    eng.state.copy_(state0); eng.obs.copy_(obs0)
    g.replay()
    torch.cuda.synchronize()
    for want, got in zip(eager, (acts, means, rec, eng.state, eng.reward, eng.terminated, eng.truncated)):
        assert torch.equal(want, got)
    eng.close()


# ---------------------------------------------------------------------------------------------- 8. full size
def test_full_size():
    env, env2, pol, b = collect_and_replay("fixedwing", "next_step", 65536, 8, offset=0)
    assert int((env.engine.flags() & L.F_NONFINITE).ne(0).sum().item()) == 0
    for key in ("obs", "actions", "mean", "reward", "logp", "advantages", "returns"):
        assert torch.isfinite(b[key]).all(), key
    env.close(); env2.close()


# ---------------------------------------------------------------------------------------------- 9. the example
def test_example_09_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "09_ppo_fixedwing_waypoints.py"), "2048", "2"], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "iteration 1" in out.stdout and "stepwise" in out.stdout

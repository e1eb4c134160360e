"""pf_rollout_policy on the device: the env part against the open-loop rollout (exact), the policy part against an fp64 forward, the
exploration noise's moments and stream, determinism / splitting, in-place parameter updates, refusals, full size, the facade."""
import ctypes as C
import math
import re
import os

import numpy as np
import pytest
import torch

from pyflyt_amd import MLPPolicy, PyFlytAmdError, build_params
from pyflyt_amd import _lib as L
from pyflyt_amd.engine import BatchEngine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, OFFSET, K = 1000, 70_001, 96  # a ragged last wave (1000 = 15 x 64 + 40), a lane offset != 0
CASES = [(t, nz, ar) for t in ("hover", "waypoints") for nz, ar in (("philox", "next_step"), ("philox", "same_step"), ("off", "next_step"))]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def engine(task="hover", noise="philox", autoreset="next_step", n=N, seed=11, offset=OFFSET, **kw):
    kw.setdefault("max_duration_seconds", 1.0)
    return BatchEngine(build_params("quadx", task, noise=noise, autoreset=autoreset, seed=seed, **kw), n, device=DEV, lane_offset=offset)


def policy(obs_dim, hidden=(64, 64), activation="tanh", log_std=-0.2, seed=5, scale=0.4):
    g = torch.Generator().manual_seed(seed)
    sizes = [obs_dim, *hidden, 4]
    ls = [((torch.randn(o, i, generator=g) * scale / math.sqrt(i) * 3.0).to(DEV).contiguous(), (torch.randn(o, generator=g) * 0.1).to(DEV))
          for i, o in zip(sizes[:-1], sizes[1:])]
    return MLPPolicy(ls, activation=activation, log_std=None if log_std is None else torch.full((4,), float(log_std), device=DEV))


def run_policy(eng, pol, k=K, step0=0, mean=True):
    out = eng.rollout_policy(pol, k, step_index0=step0, store_mean=mean)
    t = eng._traj
    res = dict(obs=out[0].clone(), reward=out[1].clone(), terminated=out[2].clone(), truncated=out[3].clone(), actions=out[4].clone(),
               state=eng.state.clone())
    if mean:
        res["mean"] = out[5].clone()
    if t["final_obs"] is not None:
        res["final_obs"], res["final_info"] = t["final_obs"].clone(), t["final_info"].clone()
    return res


def assert_same(a, b, keys=None):
    for key in keys or a.keys():
        if key in b:
            assert torch.equal(a[key], b[key]), key


@pytest.mark.parametrize("task, noise, autoreset", CASES)
def test_env_part_is_exact(task, noise, autoreset):
    """rollout_policy == rollout(actions = the actions it returned): the closed loop changes where the actions come from, nothing else."""
    e1, e2 = engine(task, noise, autoreset), engine(task, noise, autoreset)
    e1.env_reset(); e2.env_reset()
    pol = policy(e1.obs_dim, log_std=0.0)  # std 1: the drones tumble, episodes end by the dome / the floor and by the 1 s limit
    a = run_policy(e1, pol)
    o = e2.rollout(K, actions=a["actions"].clone())
    t = e2._traj
    b = dict(obs=o[0], reward=o[1], terminated=o[2], truncated=o[3], state=e2.state)
    if t["final_obs"] is not None:
        b["final_obs"], b["final_info"] = t["final_obs"], t["final_info"]
    n_done = int((a["terminated"] | a["truncated"]).sum().item())
    print(f"{task} {noise} {autoreset}: {n_done} episode ends inside the launch")
    assert n_done >= 200
    assert_same(b, a)


@pytest.mark.parametrize("task, noise, autoreset", CASES)
@pytest.mark.parametrize("hidden, activation", [((64, 64), "tanh"), ((33, 64), "relu"), ((64,), "relu"), ((1,), "tanh"), ((33,), "tanh"), ((64, 1), "tanh")])
def test_policy_part_against_fp64(task, noise, autoreset, hidden, activation):
    """mean_out[s] against the same MLP in fp64 on the recorded inputs (obs0 for s = 0, obs[s - 1] after). Bound: 8 x e32, e32 the
    largest deviation of torch's own float32 forward on the GPU from that fp64 forward on the same inputs -- the same precision,
    another summation order over at most 64 terms and another tanh. (Measured on MI355X: DESIGN.md, pf_rollout_policy.)"""
    eng = engine(task, noise, autoreset)
    obs0 = eng.env_reset().clone()
    pol = policy(eng.obs_dim, hidden, activation)
    r = run_policy(eng, pol)
    inputs = torch.cat([obs0[None], r["obs"][:-1]], 0)
    ref = pol.forward_reference(inputs, dtype=torch.float64)
    f32 = pol.forward_reference(inputs, dtype=torch.float32).double()
    e32 = (f32 - ref).abs().max().item()
    err = (r["mean"].double() - ref).abs().max().item()
    print(f"{task} {noise} {autoreset} {hidden} {activation}: kernel deviation {err:.3e}, torch float32 deviation e32 {e32:.3e}, ratio {err / e32:.2f}")
    assert err <= 8.0 * e32
    # deterministic head: the action IS the mean
    eng2 = engine(task, noise, autoreset)
    eng2.env_reset()
    det = MLPPolicy(pol.layers, activation=activation, log_std=None)
    d = run_policy(eng2, det)
    assert torch.equal(d["actions"], d["mean"])


# ---------------------------------------------------------------------------------------------- the noise
def philox_np(k0, k1, c0, c1, c2, c3):
    """Philox4x32-10 (uav_device.hpp: philox4x32) on uint32 arrays."""
    M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    c0, c1, c2, c3 = (np.asarray(x, dtype=np.uint32) + np.zeros_like(np.asarray(c0, dtype=np.uint32)) for x in (c0, c1, c2, c3))
    k0, k1 = np.uint32(k0), np.uint32(k1)
    for _ in range(10):
        p0, p1 = M0 * c0.astype(np.uint64), M1 * c2.astype(np.uint64)
        hi0, lo0, hi1, lo1 = (p0 >> np.uint64(32)).astype(np.uint32), p0.astype(np.uint32), (p1 >> np.uint64(32)).astype(np.uint32), p1.astype(np.uint32)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = np.uint32((int(k0) + 0x9E3779B9) & 0xFFFFFFFF), np.uint32((int(k1) + 0xBB67AE85) & 0xFFFFFFFF)
    return c0, c1, c2, c3


def bm16_np(w):
    """uav_device.hpp: bm16 -- one Box-Muller pair per 32-bit word from two 16-bit uniforms, in fp64."""
    u1 = ((w & np.uint32(0xFFFF)).astype(np.float64) + 0.5) / 65536.0
    u2 = (w >> np.uint32(16)).astype(np.float64) / 65536.0
    rad = np.sqrt(-2.0 * np.log(u1))
    return rad * np.cos(2 * np.pi * u2), rad * np.sin(2 * np.pi * u2)


def generator_moments():
    """The generator's own (mean, variance) over its WHOLE domain, from the numpy restatement of bm16. A normal is z = rad cos(2 pi u2)
    (or sin), rad^2 = -2 ln u1, with u1 = (i + 0.5) / 65536 and u2 = j / 65536 independent and each uniform over its 65 536 values.
    The angle grid is symmetric under u2 -> u2 + 1/2, so E[cos] = E[sin] = 0: the mean is 0. On that grid E[cos^2] = E[sin^2] = 1/2
    exactly (the sum of cos(4 pi j / 65536) over a full period is 0). Hence Var[z] = E[rad^2] E[cos^2] = mean_i(-2 ln u1_i) / 2,
    evaluated below in fp64 over all 65 536 radius draws: 1 - 5.3e-6. The bias against an ideal normal is |Var - 1|."""
    u1 = (np.arange(65536, dtype=np.float64) + 0.5) / 65536.0
    var = float(np.mean(-2.0 * np.log(u1)) * 0.5)  # E[rad^2] E[cos^2], E[cos^2] = 1/2 on the symmetric grid
    return 0.0, var


@pytest.mark.parametrize("task, noise, autoreset", CASES)
def test_noise_is_what_it_claims(task, noise, autoreset):
    eng = engine(task, noise, autoreset)
    eng.env_reset()
    ls = -0.5
    pol = policy(eng.obs_dim, log_std=ls)
    r = run_policy(eng, pol, step0=1234)
    eps = ((r["actions"].double() - r["mean"].double()) / math.exp(ls)).cpu().numpy()  # [K, N, 4]
    m = eps.size
    g_mean, g_var = generator_moments()  # the generator's bias against an ideal normal: |g_var - 1| (computed above, ~1e-5)
    bias_var = abs(g_var - 1.0)
    # float32 rounding of a = mean + std eps, read back through (a - mean) / std: at most |a| 2^-24 / std per sample; counted at its
    # full size in every moment (|a| < 8 checked here; |eps| < 5, so a second moment moves by at most 2 x 5 x that)
    assert np.abs(r["actions"].cpu().numpy()).max() < 8.0
    rnd = 8.0 * 2.0 ** -24 / math.exp(ls)
    se_mean, se_var, se_corr = 1.0 / math.sqrt(m), math.sqrt(2.0 / m), 1.0 / math.sqrt(m)
    mean, var = eps.mean(), eps.var()
    lag_steps = float(np.mean(eps[1:] * eps[:-1]))
    lag_comp = float(np.mean(eps[..., 1:] * eps[..., :-1]))
    print(f"{task} {noise} {autoreset}: n {m}, mean {mean:.3e} (6 se {6 * se_mean:.3e}), var - 1 {var - 1:.3e} (6 se {6 * se_var:.3e}, generator bias {bias_var:.3e}), "
          f"lag-1 steps {lag_steps:.3e}, components {lag_comp:.3e} (6 se {6 * se_corr:.3e})")
    assert abs(mean - g_mean) <= 6 * se_mean + rnd
    assert abs(var - 1.0) <= 6 * se_var + bias_var + 10 * rnd
    assert abs(lag_steps) <= 6 * se_corr + 10 * rnd and abs(lag_comp) <= 6 * se_corr + 10 * rnd
    # it IS the documented draw: Philox (seed, global lane, step_index0 + s, 0), stream 4, the first four normals of normal8
    seed = int(eng.params.seed)
    lanes = (OFFSET + np.arange(N)).astype(np.uint32)
    s = 7
    w = philox_np(seed & 0xFFFFFFFF, seed >> 32, lanes, np.uint32(1234 + s), np.uint32(0), np.uint32(4))
    z0, z1 = bm16_np(w[0]); z2, z3 = bm16_np(w[1])
    want = np.stack([z0, z1, z2, z3], -1)
    assert np.abs(eps[s] - want).max() < 1e-3  # (v_log / v_sin / v_cos against libm, and the read-back rounding)
    # ... and not the motor noise's normals (stream 0) nor a function of the sampled rollout's uniforms (stream 3) at the same key
    for stream in (0, 3):
        wo = philox_np(seed & 0xFFFFFFFF, seed >> 32, lanes, np.uint32(1234 + s), np.uint32(0), np.uint32(stream))
        o0, o1 = bm16_np(wo[0])
        c = np.corrcoef(np.concatenate([eps[s][:, 0], eps[s][:, 1]]), np.concatenate([o0, o1]))[0, 1]
        assert abs(c) < 6 / math.sqrt(2 * N)
    # the table in DESIGN.md names stream 4 for this draw and for no other
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    rows = re.findall(r"^\|\s*(\d)u?\s*\|([^|]*)\|", design[design.index("Philox stream constants"):], flags=re.M)
    assert [n for n, what in rows if "pf_rollout_policy" in what] == ["4"] and sorted(n for n, _ in rows) == ["0", "1", "2", "3", "4"]


@pytest.mark.parametrize("task, noise, autoreset", CASES)
def test_determinism_and_splitting(task, noise, autoreset):
    def fresh():
        e = engine(task, noise, autoreset)
        e.env_reset()
        return e, policy(e.obs_dim, log_std=0.0)

    e1, p1 = fresh()
    a = run_policy(e1, p1, step0=50)
    e2, p2 = fresh()
    b = run_policy(e2, p2, step0=50)
    assert_same(a, b)
    e3, p3 = fresh()
    h1 = run_policy(e3, p3, k=K // 2, step0=50)
    h2 = run_policy(e3, p3, k=K // 2, step0=50 + K // 2)  # (obs0: the first call's last observation row -- the engine's bookkeeping)
    for key in ("obs", "reward", "terminated", "truncated", "actions", "mean"):
        assert torch.equal(torch.cat([h1[key], h2[key]], 0), a[key]), key
    if "final_obs" in a:  # (SAME_STEP; defined where an episode ended in that step -- the other rows keep what the buffer held)
        done = a["terminated"] | a["truncated"]
        assert int(done.sum()) > 0
        for key in ("final_obs", "final_info"):
            assert torch.equal(torch.cat([h1[key], h2[key]], 0)[done], a[key][done]), key
    assert torch.equal(h2["state"], a["state"])
    e4, p4 = fresh()
    c = run_policy(e4, p4, step0=51)
    assert not torch.equal(c["actions"], a["actions"])


def test_in_place_parameter_updates_are_seen():
    eng = engine()
    eng.env_reset()
    pol = policy(eng.obs_dim, hidden=(64,), log_std=None)
    r0 = run_policy(eng, pol, k=8)
    pol.layers[0][0].mul_(0)
    r1 = run_policy(eng, pol, k=8, step0=8)
    (w0, b0), (w1, b1) = pol.layers
    want = (torch.tanh(b0.double()) @ w1.double().T + b1.double())
    assert not torch.equal(r0["mean"], r1["mean"])
    assert (r1["mean"].double() - want[None, None, :]).abs().max().item() < 1e-5
    assert torch.equal(r1["mean"][0, 0].expand_as(r1["mean"]), r1["mean"])  # one value: the biases alone


def _raises(code, fragment, fn):
    with pytest.raises(PyFlytAmdError) as e:
        fn()
    assert e.value.code == code and fragment in str(e.value), str(e.value)


def test_refusals():
    pol21 = policy(21, hidden=(8,))
    U = L.ERR_UNSUPPORTED

    def attempt(eng):  # (refused before anything is launched: no reset needed)
        return lambda: eng.rollout_policy(policy(eng.obs_dim, hidden=(8,)), 4)

    _raises(U, "QuadX-Hover and QuadX-Waypoints only", attempt(BatchEngine(build_params("fixedwing", "waypoints"), 64, device=DEV)))
    _raises(U, "flight mode 0 only", attempt(BatchEngine(build_params("quadx", "hover", flight_mode=6), 64, device=DEV)))
    _raises(U, "PF_NOISE_INJECT", attempt(BatchEngine(build_params("quadx", "hover", noise="inject"), 64, device=DEV)))
    _raises(U, "auto-reset", attempt(BatchEngine(build_params("quadx", "hover", autoreset="off"), 64, device=DEV)))
    # (shared worlds exist for the PettingZoo task only: refused as a task)
    ma = BatchEngine(build_params("quadx", "ma_hover", autoreset="off", agents_per_world=4), 64, device=DEV)
    _raises(U, "QuadX-Hover and QuadX-Waypoints only", lambda: ma.rollout_policy(policy(ma.obs_dim, hidden=(8,)), 4))
    # the generic kernel (a spawn that is not level: the specialised kernel does not take it)
    os.environ["PF_DISABLE_FAST"] = "1"
    try:
        gen = BatchEngine(build_params("quadx", "hover"), 64, device=DEV)
    finally:
        del os.environ["PF_DISABLE_FAST"]
    assert gen.lib.pf_ctx_is_specialised(gen._ctx) == 0
    _raises(U, "needs the specialised QuadX kernel", attempt(gen))
    # contact response over the 8-point manifold: the one configuration of the supported tasks without a zero-scratch instantiation
    _raises(U, "contact_manifold_points = 8", attempt(BatchEngine(build_params("quadx", "hover", world_options={"contact_manifold_points": 8}), 64, device=DEV)))
    # raw ABI: a width over 64 (MLPPolicy refuses it before the library sees it) and a given action sequence
    eng = engine()
    eng.env_reset()
    big = [torch.zeros(65, 21, device=DEV), torch.zeros(65, device=DEV), torch.zeros(4, 65, device=DEV), torch.zeros(4, device=DEV)]
    q = pol21.fill(L.PfPolicy(), eng)
    q.obs0 = eng.obs.data_ptr()
    q.width[0] = 65
    q.w[0], q.b[0], q.w[1], q.b[1] = (t.data_ptr() for t in big)
    eng.rollout(4)  # (allocates the trajectory tensors)
    t = eng._traj
    b = eng._buffers(actions_out=t["actions"])
    for name in ("obs", "reward", "terminated", "truncated"):
        setattr(b, name, t[name].data_ptr())

    def call():
        L.check(eng.lib.pf_rollout_policy(eng._ctx, C.byref(b), C.byref(q), 4, 0, eng._stream()), eng._ctx)

    _raises(U, "PF_POLICY_MAX_HIDDEN", call)
    q = pol21.fill(L.PfPolicy(), eng)
    q.obs0 = eng.obs.data_ptr()
    b.actions = t["actions"].data_ptr()
    _raises(L.ERR_ARG, "b->actions must be NULL", call)
    torch.cuda.synchronize()


@pytest.mark.parametrize("task", ["hover", "waypoints"])
@pytest.mark.parametrize("noise", ["philox", "off"])
@pytest.mark.parametrize("points", [4, 8])
def test_contact_response_off_is_supported(task, noise, points):
    """Contexts without the contact response (either manifold) run their own instantiations: the env part exact, as above."""
    kw = dict(world_options={"contact_response": False, "contact_manifold_points": points})
    e1, e2 = engine(task, noise, **kw), engine(task, noise, **kw)
    e1.env_reset(); e2.env_reset()
    pol = policy(e1.obs_dim, log_std=0.0)
    a = run_policy(e1, pol)
    o = e2.rollout(K, actions=a["actions"].clone())
    assert int((a["terminated"] | a["truncated"]).sum().item()) >= 200
    for key, v in zip(("obs", "reward", "terminated", "truncated"), o):
        assert torch.equal(v, a[key]), key
    assert torch.equal(e2.state, a["state"])
    ref = pol.forward_reference(a["obs"][:-1], dtype=torch.float64)  # (the means follow the observations here as well)
    assert (a["mean"][1:].double() - ref).abs().max().item() < 1e-4


def test_example_05_runs():
    import subprocess
    import sys

    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "05_policy_rollout.py"), "4096"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "100 policy steps" in out.stdout


def test_full_size():
    n, k = 65536, 20
    e1, e2 = engine(n=n, offset=0), engine(n=n, offset=0)
    e1.env_reset(); e2.env_reset()
    pol = policy(e1.obs_dim, log_std=0.0)
    a = run_policy(e1, pol, k=k)
    o = e2.rollout(k, actions=a["actions"].clone())
    for key, v in zip(("obs", "reward", "terminated", "truncated"), o):
        assert torch.equal(v, a[key]), key
    assert torch.equal(e2.state, a["state"])
    assert int((e1.flags() & L.F_NONFINITE).ne(0).sum().item()) == 0
    assert torch.isfinite(a["obs"]).all() and torch.isfinite(a["actions"]).all()


def test_facade_rollout():
    from pyflyt_amd.gym_envs import make_vec

    env = make_vec("PyFlyt/QuadX-Hover-v4", 4096, seed=3)
    env.reset()
    pol = policy(env.engine.obs_dim)
    r1 = [x.clone() for x in env.rollout(pol, 50)[:5]]
    out2 = env.rollout(pol, 50)
    r2, infos = [x.clone() for x in out2[:5]], out2[5]
    eng = BatchEngine(env.engine.params, 4096, device=DEV, lane_offset=env.engine.lane_offset)
    eng.env_reset()
    full = eng.rollout_policy(pol, 100)
    for x1, x2, f in zip(r1, r2, full):
        assert torch.equal(torch.cat([x1, x2], 0), f)
    assert torch.equal(env.engine.state, eng.state)
    flags = eng.flags()
    assert torch.equal(infos["collision"], (flags & L.F_INFO_COLLISION) != 0)
    assert torch.equal(infos["out_of_bounds"], (flags & L.F_INFO_OOB) != 0)
    env.close()

"""pf_traj_stats and env.collect(stats=True) on the device, against a numpy restatement of the contract in include/pyflyt_amd.h
(written from the contract, not from the kernels): the per-lane float32 recursions bit for bit, the double sums and the running
moments within the rounding bound of their sums, NaN poisoning of everything that must not be selected, splitting, merging,
lane-count independence, collect end to end, resets, graph capture, the error paths, the example."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from pyflyt_amd import MLPPolicy, RunningMoments, build_params
from pyflyt_amd import _lib as L
from pyflyt_amd.engine import BatchEngine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 200  # four waves, the last one partial (3 x 64 + 8)
U64 = 2.0 ** -53
MODES = ("next_step", "same_step")
TASKS = ("hover", "waypoints")


# ---------------------------------------------------------------------------------------------- the reference
def fma32(a, b, c):
    """fma(a, b, c) in float32, rounded ONCE. a * b is exact in float64 (two 24-bit significands); p + c is rounded to float64 and
    then to float32, which differs from the single rounding only when the float64 sum lies exactly half way between two float32
    numbers while the exact sum does not: TwoSum gives the exact residual e, and its sign breaks that tie."""
    p = np.float64(a) * b.astype(np.float64)
    c64 = c.astype(np.float64)
    s = p + c64
    bb = s - p
    e = (p - (s - bb)) + (c64 - bb)
    f = s.astype(np.float32)
    d = s - f.astype(np.float64)
    other = np.nextafter(f, np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)))
    tie = (d != 0) & (np.abs(d) == np.abs(other.astype(np.float64) - s)) & (np.sign(e) == np.sign(d))
    return np.where(tie, other, f).astype(np.float32)


def ref_traj(mode, gamma, reward, terminated, truncated, episode_start=None, carry=None):
    """The per-lane recursion, sequential in s, float32 as the contract fixes it. Returns the per-step outputs, valid, the G of every
    step (what ret_moments is taken over, on valid steps), the carries after the call and summary."""
    k, n = reward.shape
    g = np.float32(gamma)
    ret, ln, G = (x.copy() for x in carry) if carry is not None else (np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.float32))
    term, trunc = terminated.astype(bool), truncated.astype(bool)
    prev = episode_start.astype(bool) if (mode == "next_step" and episode_start is not None) else np.zeros(n, dtype=bool)
    ep_ret, ep_len = np.zeros((k, n), np.float32), np.zeros((k, n), np.int32)
    valid, Gs, fins = np.ones((k, n), dtype=bool), np.zeros((k, n), np.float32), np.zeros((k, n), dtype=bool)
    with np.errstate(invalid="ignore"):
        for s in range(k):
            done = term[s] | trunc[s]
            v = ~prev if mode == "next_step" else np.ones(n, dtype=bool)
            ret = np.where(v, (ret + reward[s]).astype(np.float32), ret)
            ln = np.where(v, ln + 1, ln).astype(np.int32)
            G = np.where(v, fma32(g, G, reward[s]), G)
            valid[s], Gs[s] = v, G
            fin = v & done
            fins[s] = fin
            ep_ret[s], ep_len[s] = np.where(fin, ret, np.float32(0)), np.where(fin, ln, 0)
            ret, ln, G = np.where(fin, np.float32(0), ret), np.where(fin, 0, ln).astype(np.int32), np.where(fin, np.float32(0), G)
            prev = done
    r64 = ep_ret[fins].astype(np.float64)
    c = int(fins.sum())
    summary = np.array([c, r64.sum(), (r64 * r64).sum(), r64.min() if c else np.inf, r64.max() if c else -np.inf, ep_len[fins].sum(),
                        (fins & term).sum(), (fins & ~term).sum()], dtype=np.float64)
    return dict(ep_ret=ep_ret, ep_len=ep_len, valid=valid, G=Gs, fin=fins, carry=(ret, ln, G), summary=summary)


def ref_moments(x):
    """(count, mean, M2) of the rows of x [m, D] in float64."""
    x = x.astype(np.float64)
    if x.shape[0] == 0:
        return 0.0, np.zeros(x.shape[1]), np.zeros(x.shape[1])
    mean = x.mean(0)
    return float(x.shape[0]), mean, ((x - mean) ** 2).sum(0)


def gamma_n(terms):
    return terms * U64 / (1.0 - terms * U64)


def sum_bound(terms, t):
    """|fl(sum t_i) - sum t_i| <= gamma_N sum |t_i| for an N-term double sum in ANY order (Higham, Accuracy and Stability, (4.4))."""
    return gamma_n(terms) * float(np.abs(t).sum())


def moments_bound(rows, x, shift, m2_before):
    """The error of one call's update of (mean, M2), per column, for its valid samples x [m, D] and the mean `shift` the block held
    before it; `rows` = k n, the terms of each sum (the unselected ones are exact zeros). With d_i = x_i - shift, T1 = sum |d_i|,
    T2 = sum d_i^2 and g = gamma_(rows + 8) (the sum, the at most three roundings inside a term, and the handful of operations of the merge):
      S1 = sum d_i is off by at most g T1, S2 = sum d_i^2 by g T2.
      mean = shift + (S1 / nb)(nb / tot): off by at most g (T1 / nb + |shift|).
      M2 = M2_a + (S2 - S1^2 / nb) + (S1 / nb)^2 na nb / tot: S1^2 / nb is off by (2 |S1| g T1 + (g T1)^2) / nb <= 2 g T2 (1 + g)
      because T1^2 <= nb T2 (Cauchy-Schwarz); the last term is at most S1^2 / nb and carries the same error; the additions round
      quantities no larger than M2_a + 3 T2. Together at most g (8 T2 + M2_a).
    The float64 numpy reference sums the same terms and is itself off by no more than that, hence the factor 2."""
    if x.shape[0] == 0:
        return np.zeros(x.shape[1]), np.zeros(x.shape[1])
    d = x.astype(np.float64) - shift
    g = gamma_n(rows + 8)
    t1, t2 = np.abs(d).sum(0), (d * d).sum(0)
    return 2.0 * g * (t1 / x.shape[0] + np.abs(shift)), 2.0 * g * (8.0 * t2 + m2_before)


def synth(mode, k, n=N, seed=0, D=None):
    """Random rewards, done with probability about 0.1 (terminated and truncated both, sometimes together), some episode_start; lane
    0 finishes at s = 0, lane 1 at s = k - 1, lane 2 twice where k admits it. Under NEXT_STEP the step after a finished one is a
    reset step as pf_env_step writes it: reward 0 and both flags 0."""
    rng = np.random.default_rng(77 * k + seed)
    term = rng.random((k, n)) < 0.06
    trunc = rng.random((k, n)) < 0.06
    term[:, :4] = False
    trunc[:, :4] = False
    term[0, 0] = True
    trunc[k - 1, 1] = True
    gap = 2 if mode == "next_step" else 1
    if k > gap:
        term[0, 2] = True
        trunc[gap, 2] = True
    reward = (rng.normal(size=(k, n)) * 2.0 + 0.5).astype(np.float32)
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
    d = dict(reward=reward, terminated=term, truncated=trunc, episode_start=episode_start)
    if D is not None:  # columns with different offsets and scales
        d["obs"] = (rng.normal(size=(k, n, D)) * np.linspace(0.1, 3.0, D) + np.linspace(-2.0, 5.0, D)).astype(np.float32)
    return d


def engine(mode, n=N, task="hover"):
    return BatchEngine(build_params("quadx", task, autoreset=mode, seed=3), n, device=DEV)


def dev(x):
    return None if x is None else torch.as_tensor(x, device=DEV).contiguous()


def run(eng, d, gamma=0.99, store_steps=True):
    er, el, summ = eng.traj_stats(dev(d["reward"]), dev(d["terminated"]), dev(d["truncated"]), gamma=gamma, episode_start=dev(d.get("episode_start")),
                                  obs=dev(d.get("obs")), store_steps=store_steps)
    torch.cuda.synchronize()
    ts = eng._traj_state()
    return dict(ep_ret=None if er is None else er.cpu().numpy().copy(), ep_len=None if el is None else el.cpu().numpy().copy(),
                summary=summ.cpu().numpy().copy(), carry=tuple(ts[key].cpu().numpy().copy() for key in ("carry_return", "carry_length", "carry_disc")),
                ret_moments=ts["ret_moments"].cpu().numpy().copy(), obs_moments=ts["obs_moments"].cpu().numpy().copy())


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype.itemsize == 4 else np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def check_lanes(got, ref):
    assert same_bits(got["ep_ret"], ref["ep_ret"]) and np.array_equal(got["ep_len"], ref["ep_len"]) and got["ep_len"].dtype == np.int32
    for name, g, r in zip(("carry_return", "carry_length", "carry_disc"), got["carry"], ref["carry"]):
        assert same_bits(g, r), name


def check_summary(got, ref, rows):
    s, r = got["summary"], ref["summary"]
    for j in (0, 3, 4, 5, 6, 7):  # counts, min, max, the whole-number sum of lengths: exact
        assert s[j] == r[j], (j, s[j], r[j])
    er = ref["ep_ret"][ref["fin"]].astype(np.float64)
    b1, b2 = 2.0 * sum_bound(rows, er), 2.0 * sum_bound(rows, er * er)  # (2: the reference's own sum)
    print(f"summary: sum of returns off by {abs(s[1] - r[1]):.3e} (bound {b1:.3e}), of squares by {abs(s[2] - r[2]):.3e} (bound {b2:.3e})")
    assert abs(s[1] - r[1]) <= b1 and abs(s[2] - r[2]) <= b2


def check_moments(block, samples, bounds, what):
    """block: (count, mean[D], M2[D]) from the device; samples: every valid sample it should hold [m, D]; bounds: the summed per-call bounds."""
    D = samples.shape[1]
    cnt, mean, m2 = ref_moments(samples)
    em, e2 = np.abs(block[1:1 + D] - mean), np.abs(block[1 + D:] - m2)
    print(f"{what}: count {block[0]:.0f}, mean off by {em.max():.3e} (bound {bounds[0].max():.3e}), M2 by {e2.max():.3e} (bound {bounds[1].max():.3e})")
    assert block[0] == cnt
    assert (em <= bounds[0]).all() and (e2 <= bounds[1]).all()


# ---------------------------------------------------------------------------------------------- 1. synthetic trajectories
@pytest.mark.parametrize("task", TASKS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [1, 7, 37])
def test_synthetic_trajectories(task, mode, k):
    eng = engine(mode, task=task)
    D = eng.obs_dim
    assert D == 21 if task == "hover" else D > 21
    d = synth(mode, k, D=D)
    ref = ref_traj(mode, 0.99, d["reward"], d["terminated"], d["truncated"], d["episode_start"])
    done = d["terminated"] | d["truncated"]
    # the inputs exercise the contract
    if k > (2 if mode == "next_step" else 1):
        assert (ref["fin"].sum(0) >= 2).any()
    assert done[k - 1].any() and ref["fin"][k - 1].any()
    assert d["terminated"].any() and d["truncated"].any()
    if mode == "next_step":
        assert d["episode_start"].any() and (~ref["valid"]).any()
    else:
        assert ref["valid"].all()
    got = run(eng, d)
    check_lanes(got, ref)
    check_summary(got, ref, k * N)
    v = ref["valid"]
    zero = np.zeros(1)
    check_moments(got["ret_moments"], ref["G"][v][:, None], moments_bound(k * N, ref["G"][v][:, None], zero, zero), "ret_moments")
    check_moments(got["obs_moments"], d["obs"][v], moments_bound(k * N, d["obs"][v], np.zeros(D), np.zeros(D)), "obs_moments")
    # without the per-step outputs and the observations: the same carries and summary, the observation block untouched
    eng2 = engine(mode, task=task)
    d2 = {key: val for key, val in d.items() if key != "obs"}
    got2 = run(eng2, d2, store_steps=False)
    assert got2["ep_ret"] is None and got2["ep_len"] is None
    assert same_bits(got2["summary"], got["summary"]) and same_bits(got2["ret_moments"], got["ret_moments"])
    assert all(same_bits(a, b) for a, b in zip(got2["carry"], got["carry"])) and not got2["obs_moments"].any()
    eng.close(); eng2.close()


# ---------------------------------------------------------------------------------------------- 2. poison
@pytest.mark.parametrize("k", [7, 37])
def test_poison_in_invalid_steps_reaches_nothing(k):
    d = synth("next_step", k, seed=1, D=21)
    ref = ref_traj("next_step", 0.99, d["reward"], d["terminated"], d["truncated"], d["episode_start"])
    inv = ~ref["valid"]
    assert inv.any()
    e1, e2 = engine("next_step"), engine("next_step")
    clean = run(e1, d)
    p = {key: val.copy() for key, val in d.items()}
    p["reward"][inv] = np.nan
    p["obs"][inv] = np.nan
    dirty = run(e2, p)
    for key in ("ep_ret", "ep_len", "summary", "ret_moments", "obs_moments"):
        assert np.isfinite(dirty[key][np.isfinite(clean[key])]).all() and same_bits(clean[key], dirty[key]), key
    for a, b in zip(clean["carry"], dirty["carry"]):
        assert same_bits(a, b)
    e1.close(); e2.close()
    # SAME_STEP has no invalid step: nothing to poison
    s = synth("same_step", k, seed=1)
    assert ref_traj("same_step", 0.99, s["reward"], s["terminated"], s["truncated"])["valid"].all()


# ---------------------------------------------------------------------------------------------- 2b. the unrolled loop of the observation kernel
@pytest.mark.parametrize("mode", MODES)
def test_observation_moments_beyond_one_pass_of_the_grid(mode):
    """The observation kernel's grid is capped at 1024 blocks of 256 threads and a thread takes eight rows per pass of its main loop:
    the cases above (k n D < 8 x 1024 x 256 floats) never enter that loop. n = 4096, k = 37, D = 21 is 3.18 M floats: every thread runs
    the eight-row body once and a tail of four or five rows (151 552 rows, 12 483 rows per stride). Under NEXT_STEP with NaN in every
    invalid row and reward."""
    n, k, D = 4096, 37, 21
    grid_threads = 1024 * 256
    rows, row_step = n * k, grid_threads // D
    assert rows * D > 8 * grid_threads and rows > 8 * row_step and rows % (8 * row_step) > row_step  # the main loop AND a tail
    d = synth(mode, k, n=n, seed=8, D=D)
    ref = ref_traj(mode, 0.99, d["reward"], d["terminated"], d["truncated"], d["episode_start"])
    v = ref["valid"]
    if mode == "next_step":
        assert (~v).sum() > 1000 and (~v[0]).any() and (~v[1:]).any()
        d["reward"][~v] = np.nan
        d["obs"][~v] = np.nan
    else:
        assert v.all()
    eng = engine(mode, n=n)
    got = run(eng, d)
    check_lanes(got, ref)
    check_summary(got, ref, rows)
    assert np.isfinite(got["obs_moments"]).all() and np.isfinite(got["ret_moments"]).all()
    check_moments(got["obs_moments"], d["obs"][v], moments_bound(rows, d["obs"][v], np.zeros(D), np.zeros(D)), "obs_moments")
    check_moments(got["ret_moments"], ref["G"][v][:, None], moments_bound(rows, ref["G"][v][:, None], np.zeros(1), np.zeros(1)), "ret_moments")
    # a second batch into the same block: the shift is now the running mean
    d2 = synth(mode, k, n=n, seed=9, D=D)
    r2 = ref_traj(mode, 0.99, d2["reward"], d2["terminated"], d2["truncated"], d2["episode_start"], carry=ref["carry"])
    got2 = run(eng, d2)
    check_lanes(got2, r2)
    mid = got["obs_moments"]
    b1 = moments_bound(rows, d["obs"][v], np.zeros(D), np.zeros(D))
    b2 = moments_bound(rows, d2["obs"][r2["valid"]], mid[1:1 + D], mid[1 + D:])
    check_moments(got2["obs_moments"], np.concatenate([d["obs"][v], d2["obs"][r2["valid"]]]), (b1[0] + b2[0], b1[1] + b2[1]), "obs_moments (two batches)")
    eng.close()


# ---------------------------------------------------------------------------------------------- 3. splitting, 4. the running merge
def halves(mode, d, k):
    h = k // 2
    a = {key: (val[:h] if key != "episode_start" else val) for key, val in d.items() if val is not None}
    b = {key: val[h:] for key, val in d.items() if val is not None and key != "episode_start"}
    if mode == "next_step":
        b["episode_start"] = d["terminated"][h - 1] | d["truncated"][h - 1]
    return a, b


@pytest.mark.parametrize("mode", MODES)
def test_splitting_a_call(mode):
    k, D = 36, 21
    d = synth(mode, k, seed=2, D=D)
    ref = ref_traj(mode, 0.99, d["reward"], d["terminated"], d["truncated"], d["episode_start"])
    whole, split = engine(mode), engine(mode)
    w = run(whole, d)
    a, b = halves(mode, d, k)
    ga = run(split, a)
    mid = ga["obs_moments"].copy(), ga["ret_moments"].copy()
    gb = run(split, b)
    assert same_bits(np.concatenate([ga["ep_ret"], gb["ep_ret"]]), w["ep_ret"]) and same_bits(w["ep_ret"], ref["ep_ret"])
    assert np.array_equal(np.concatenate([ga["ep_len"], gb["ep_len"]]), w["ep_len"])
    for x, y, z in zip(gb["carry"], w["carry"], ref["carry"]):
        assert same_bits(x, y) and same_bits(x, z)
    assert ga["summary"][0] + gb["summary"][0] == w["summary"][0] and min(ga["summary"][3], gb["summary"][3]) == w["summary"][3]
    v, h = ref["valid"], k // 2
    zero = np.zeros(1)
    for name, samples, mids in (("obs_moments", d["obs"], mid[0]), ("ret_moments", ref["G"][..., None], mid[1])):
        Dm = samples.shape[-1]
        allv, first, second = samples[v], samples[:h][v[:h]], samples[h:][v[h:]]
        bw = moments_bound(k * N, allv, np.zeros(Dm), np.zeros(Dm))
        b1 = moments_bound(h * N, first, np.zeros(Dm), np.zeros(Dm))
        b2 = moments_bound(h * N, second, mids[1:1 + Dm], mids[1 + Dm:])
        check_moments(w[name], allv, bw, name + " (one call)")
        check_moments(gb[name], allv, (b1[0] + b2[0], b1[1] + b2[1]), name + " (two calls)")
    # a repeated identical call: the same bits in summary and moments
    ts = split._traj_state()
    keep = {key: ts[key].clone() for key in ("carry_return", "carry_length", "carry_disc", "obs_moments", "ret_moments")}
    r1 = run(split, a)
    for key, val in keep.items():
        ts[key].copy_(val)
    r2 = run(split, a)
    for key in ("summary", "ret_moments", "obs_moments", "ep_ret", "ep_len"):
        assert same_bits(r1[key], r2[key]), key
    whole.close(); split.close()


@pytest.mark.parametrize("mode", MODES)
def test_two_batches_merge_into_the_moments_of_their_concatenation(mode):
    D = 21
    d1, d2 = synth(mode, 7, seed=3, D=D), synth(mode, 37, seed=4, D=D)
    d2["obs"] = (d2["obs"] * 1.5 + 3.0).astype(np.float32)  # (another distribution: the merge has a delta to carry)
    d2["reward"] = (d2["reward"] - 2.0).astype(np.float32) * (d2["reward"] != 0)
    eng = engine(mode)
    r1 = ref_traj(mode, 0.99, d1["reward"], d1["terminated"], d1["truncated"], d1["episode_start"])
    g1 = run(eng, d1)
    r2 = ref_traj(mode, 0.99, d2["reward"], d2["terminated"], d2["truncated"], d2["episode_start"], carry=r1["carry"])
    g2 = run(eng, d2)
    check_lanes(g2, r2)
    for name, s1, s2, mid in (("obs_moments", d1["obs"][r1["valid"]], d2["obs"][r2["valid"]], g1["obs_moments"]),
                              ("ret_moments", r1["G"][r1["valid"]][:, None], r2["G"][r2["valid"]][:, None], g1["ret_moments"])):
        Dm = s1.shape[1]
        b1 = moments_bound(7 * N, s1, np.zeros(Dm), np.zeros(Dm))
        b2 = moments_bound(37 * N, s2, mid[1:1 + Dm], mid[1 + Dm:])
        check_moments(g2[name], np.concatenate([s1, s2]), (b1[0] + b2[0], b1[1] + b2[1]), name)
    rm = RunningMoments(eng.obs_moments)
    cnt, mean, m2 = ref_moments(np.concatenate([d1["obs"][r1["valid"]], d2["obs"][r2["valid"]]]))
    assert rm.mean.dtype == torch.float32 and rm.mean.device.type == "cuda" and float(rm.count) == cnt
    assert np.allclose(rm.mean.cpu().numpy(), mean, rtol=1e-6, atol=1e-6) and np.allclose(rm.var.cpu().numpy(), m2 / cnt, rtol=1e-6)
    eng.reset_moments()
    assert not eng.obs_moments.any() and not eng.ret_moments.any() and eng._traj_state()["carry_length"].any()
    eng.close()


# ---------------------------------------------------------------------------------------------- 5. lane-count independence
@pytest.mark.parametrize("mode", MODES)
def test_lanes_do_not_depend_on_the_lane_count(mode):
    k = 37
    big = synth(mode, k, n=256, seed=5)
    small = {key: (None if val is None else np.ascontiguousarray(val[..., :N])) for key, val in big.items()}
    e1, e2 = engine(mode, n=N), engine(mode, n=256)
    a, b = run(e1, small), run(e2, big)
    assert same_bits(a["ep_ret"], np.ascontiguousarray(b["ep_ret"][:, :N])) and np.array_equal(a["ep_len"], b["ep_len"][:, :N])
    for x, y in zip(a["carry"], b["carry"]):
        assert same_bits(x, np.ascontiguousarray(y[:N]))
    e1.close(); e2.close()


# ---------------------------------------------------------------------------------------------- 6. collect end to end
def make_env(task, mode, n=256, seed=11):
    from pyflyt_amd.gym_envs import make_vec

    env_id = "PyFlyt/QuadX-Hover-v4" if task == "hover" else "PyFlyt/QuadX-Waypoints-v4"
    return make_vec(env_id, n, seed=seed, autoreset_mode=mode, max_duration_seconds=0.5)


def make_nets(obs_dim):
    g = torch.Generator().manual_seed(5)
    sizes = [obs_dim, 64, 64, 4]
    ls = [((torch.randn(o, i, generator=g) * 1.2 / math.sqrt(i)).to(DEV).contiguous(), (torch.randn(o, generator=g) * 0.1).to(DEV))
          for i, o in zip(sizes[:-1], sizes[1:])]
    pol = MLPPolicy(ls, log_std=torch.zeros(4, device=DEV))
    torch.manual_seed(7)
    nn = torch.nn
    vnet = nn.Sequential(nn.Linear(obs_dim, 32), nn.Tanh(), nn.Linear(32, 1)).to(DEV)
    return pol, vnet


TODAYS_KEYS = {"obs", "actions", "mean", "logp", "values", "advantages", "returns", "valid", "reward", "terminated", "truncated", "last_value", "infos"}


@pytest.mark.parametrize("task", TASKS)
@pytest.mark.parametrize("mode", MODES)
def test_collect_with_stats_end_to_end(task, mode):
    k, n, gamma = 64, 256, 0.99
    env = make_env(task, mode)
    env.reset()
    D = env.engine.obs_dim
    pol, vnet = make_nets(D)
    seen = []

    def value_fn(o):
        seen.append(vnet(o))
        return seen[-1]

    es = ((env.engine.flags() & 3) != 0).cpu().numpy()
    b = env.collect(pol, value_fn, k, gamma=gamma, stats=True)
    torch.cuda.synchronize()
    assert set(b.keys()) == TODAYS_KEYS | {"episode_return", "episode_length", "episode_summary"}
    rew, term, trunc = b["reward"].cpu().numpy(), b["terminated"].cpu().numpy(), b["truncated"].cpu().numpy()
    ref = ref_traj(mode, gamma, rew, term, trunc, es if mode == "next_step" else None)
    # the time limit guarantees that every lane finishes at least two episodes whatever the policy does
    per_lane = ref["fin"].sum(0)
    print(f"{task} {mode}: {int(ref['fin'].sum())} episodes, at least {int(per_lane.min())} per lane, {int(term.sum())} terminations, {int(trunc.sum())} truncations")
    assert per_lane.min() >= 2
    assert same_bits(b["episode_return"].cpu().numpy(), ref["ep_ret"]) and np.array_equal(b["episode_length"].cpu().numpy(), ref["ep_len"])
    assert np.array_equal(b["valid"].cpu().numpy(), ref["valid"])
    ts = env.engine._traj_state()
    got = dict(summary=b["episode_summary"].cpu().numpy(), carry=tuple(ts[key].cpu().numpy() for key in ("carry_return", "carry_length", "carry_disc")))
    for x, y in zip(got["carry"], ref["carry"]):
        assert same_bits(x, y)
    check_summary(got, ref, k * n)
    v = ref["valid"]
    obs = b["obs"].cpu().numpy()
    check_moments(env.obs_rms.block.cpu().numpy(), obs[v], moments_bound(k * n, obs[v], np.zeros(D), np.zeros(D)), "obs_rms")
    check_moments(env.ret_rms.block.cpu().numpy(), ref["G"][v][:, None], moments_bound(k * n, ref["G"][v][:, None], np.zeros(1), np.zeros(1)), "ret_rms")
    sd = env.episode_summary_dict()
    assert sd["episodes"] == int(ref["fin"].sum()) and sd["terminated"] + sd["truncated"] == sd["episodes"]
    assert math.isclose(sd["return_mean"], float(ref["ep_ret"][ref["fin"]].astype(np.float64).mean()), rel_tol=1e-9, abs_tol=1e-9)
    assert math.isclose(sd["length_mean"], float(ref["ep_len"][ref["fin"]].mean()), rel_tol=1e-12)
    # normalize_reward: pf_gae gets the scaled reward, computed with the moments AFTER this batch's update; reward stays raw
    seen.clear()
    last_done = (b["terminated"][-1] | b["truncated"][-1]).clone()  # (b's tensors are the engine's: the next collect overwrites them)
    b2 = env.collect(pol, value_fn, k, gamma=gamma, normalize_reward=True)
    assert set(b2.keys()) == TODAYS_KEYS | {"episode_return", "episode_length", "episode_summary", "reward_scaled"}
    scaled = b2["reward"] / (env.ret_rms.var + 1e-8).sqrt()
    assert torch.equal(b2["reward_scaled"], scaled) and float(env.ret_rms.count) > float(v.sum())
    adv, ret = b2["advantages"].clone(), b2["returns"].clone()
    values = torch.cat([b2["values"], b2["last_value"][None]], 0).contiguous()
    fv = seen[1].reshape(k, n).contiguous() if mode == "same_step" else None
    es2 = last_done if mode == "next_step" else None
    a2, r2, _, _ = env.engine.gae(b2["reward_scaled"], b2["terminated"], b2["truncated"], values, gamma=gamma, lam=0.95, final_values=fv, episode_start=es2)
    assert torch.equal(a2, adv) and torch.equal(r2, ret)
    # the default call is today's
    b3 = env.collect(pol, value_fn, k, gamma=gamma)
    assert set(b3.keys()) == TODAYS_KEYS
    env.close()


# ---------------------------------------------------------------------------------------------- 7. resets
def test_resets_zero_the_carries_and_keep_the_moments():
    env = make_env("hover", "next_step", n=128)
    env.reset()
    pol, vnet = make_nets(env.engine.obs_dim)
    env.collect(pol, vnet, 7, stats=True)  # (7 steps of a 20-step episode: every lane's episode is open)
    ts = env.engine._traj_state()
    before = {key: ts[key].clone() for key in ("carry_return", "carry_length", "carry_disc")}
    assert (before["carry_length"] > 0).float().mean() > 0.9 and (before["carry_return"] != 0).float().mean() > 0.9
    mask = torch.zeros(128, dtype=torch.bool, device=DEV)
    mask[5:70] = True
    env.reset(options={"reset_mask": mask})
    for key, was in before.items():
        assert was[mask].any() and not ts[key][mask].any() and torch.equal(ts[key][~mask], was[~mask]), key
    moments = env.obs_rms.block.clone(), env.ret_rms.block.clone()
    assert 0 < moments[0][0] <= 7 * 128
    env.reset(seed=11)  # the same seed: the same engine
    assert not any(ts[key].any() for key in before)
    assert torch.equal(env.obs_rms.block, moments[0]) and torch.equal(env.ret_rms.block, moments[1])
    env.collect(pol, vnet, 7, stats=True)
    moments = env.obs_rms.block.clone(), env.ret_rms.block.clone()
    env.reset(seed=12)  # another seed: a new engine
    ts = env.engine._traj_state()
    assert not any(ts[key].any() for key in before)
    assert moments[0][0] > 7 * 128 and torch.equal(env.obs_rms.block, moments[0]) and torch.equal(env.ret_rms.block, moments[1])
    env.close()


# ---------------------------------------------------------------------------------------------- 8. graph capture
def test_traj_stats_is_capturable():
    mode, k = "next_step", 20
    d = synth(mode, k, seed=6, D=21)
    t = {key: dev(val) for key, val in d.items()}
    eng = engine(mode)
    ts = eng._traj_state()
    state = ("carry_return", "carry_length", "carry_disc", "obs_moments", "ret_moments")

    def call():
        return eng.traj_stats(t["reward"], t["terminated"], t["truncated"], gamma=0.99, episode_start=t["episode_start"], obs=t["obs"])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = [x.clone() for x in out] + [ts[key].clone() for key in state]
    for key in state:
        ts[key].zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    for x in out:
        x.zero_()
    for key in state:
        ts[key].zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(list(out) + [ts[key] for key in state], eager):
        assert same_bits(x.cpu().numpy(), y.cpu().numpy())
    assert float(eager[2][0]) > 0 and float(eager[0].abs().sum()) > 0
    eng.close()


# ---------------------------------------------------------------------------------------------- 9. error paths
def test_error_paths_name_the_argument():
    k, n = 4, 64
    for mode in ("next_step", "same_step", "off"):
        eng = engine(mode, n=n)
        D = eng.obs_dim
        f32, f64 = dict(dtype=torch.float32, device=DEV), dict(dtype=torch.float64, device=DEV)
        buf = dict(reward=torch.zeros(k, n, **f32), terminated=torch.zeros(k, n, dtype=torch.bool, device=DEV),
                   truncated=torch.zeros(k, n, dtype=torch.bool, device=DEV), episode_start=torch.zeros(n, dtype=torch.bool, device=DEV),
                   obs=torch.zeros(k, n, D, **f32), carry_return=torch.zeros(n, **f32), carry_length=torch.zeros(n, dtype=torch.int32, device=DEV),
                   carry_disc=torch.zeros(n, **f32), ep_return_out=torch.zeros(k, n, **f32),
                   ep_length_out=torch.zeros(k, n, dtype=torch.int32, device=DEV), summary=torch.zeros(8, **f64),
                   ret_moments=torch.zeros(3, **f64), obs_moments=torch.zeros(1 + 2 * D, **f64))

        def block(**change):
            a = L.PfTrajStats()
            a.gamma, vals = 0.99, dict(buf)
            if mode != "next_step":
                vals["episode_start"] = None
            for key, v in {**vals, **change}.items():
                setattr(a, key, v if isinstance(v, float) or v is None else v.data_ptr())
            return a

        def refused(fragment, steps=k, **change):
            rc = eng.lib.pf_traj_stats(eng._ctx, C.byref(block(**change)), steps, eng._stream())
            msg = eng.lib.pf_last_error(eng._ctx).decode()
            assert rc == L.ERR_ARG and fragment in msg, (rc, msg)

        assert eng.lib.pf_traj_stats(eng._ctx, C.byref(block()), k, eng._stream()) == 0  # (the unchanged block is accepted)
        assert eng.lib.pf_traj_stats(eng._ctx, C.byref(block(ep_return_out=None, ep_length_out=None, ret_moments=None, obs=None, obs_moments=None)), k,
                                     eng._stream()) == 0  # (and so is one without anything optional)
        refused("k_steps", steps=0)
        for name in ("reward", "terminated", "truncated", "summary", "carry_return", "carry_length", "carry_disc"):
            refused(name, **{name: None})
        refused("gamma", gamma=1.5)
        refused("gamma", gamma=-0.5)
        refused("gamma", gamma=float("nan"))
        if mode != "next_step":
            refused("episode_start", episode_start=buf["episode_start"])
        refused("obs comes with obs_moments", obs_moments=None)
        refused("obs_moments comes with obs", obs=None)
        torch.cuda.synchronize()
        with pytest.raises(ValueError, match="obs must be a contiguous float32 tensor of shape"):
            eng.traj_stats(buf["reward"], buf["terminated"], buf["truncated"], obs=torch.zeros(k, n, D + 1, **f32))
        eng.close()
    aviary = BatchEngine(build_params("quadx", "none"), 64, device=DEV)
    rc = aviary.lib.pf_traj_stats(aviary._ctx, C.byref(L.PfTrajStats()), 4, aviary._stream())
    assert rc == L.ERR_UNSUPPORTED and "env task" in aviary.lib.pf_last_error(aviary._ctx).decode()
    aviary.close()


# ---------------------------------------------------------------------------------------------- 10. the example
def test_example_07_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "07_ppo_hover_normalized.py"), "1024", "2"], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = re.findall(r"(\d+) episodes finished, mean episode return ([-+0-9.eE]+|nan|inf), mean episode length ([-+0-9.eE]+|nan|inf)", out.stdout)
    assert len(rows) == 2 and all(int(r[0]) > 0 and math.isfinite(float(r[1])) and float(r[2]) > 0 for r in rows), out.stdout

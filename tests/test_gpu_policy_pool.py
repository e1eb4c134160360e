"""pf_policy_pool_plan / pf_policy_act_pool on the device: every row against the one-policy launch bit for bit, the means against fp64,
graph capture, the dogfight's pooled closed loop against the unpooled one, its launch sequence, lists of policies on the vector envs
against a hand-written loop, the example."""
import os
import subprocess
import sys

import pytest
import torch

from pyflyt_amd import MLPPolicy
from pyflyt_amd import _lib as L
from pyflyt_amd.gym_envs.vector_envs import FixedwingWaypointsVecEnv, QuadXHoverVecEnv
from pyflyt_amd.pz_envs import MAFixedwingDogfightEnv
from test_gpu_launch_sequence import K as SEQ_K, STEP0, recorded  # (Recorder, through recorded(): imported, not edited)
from test_gpu_ma_collect import env_policy, make_env
from test_gpu_policy_act import N, net, other_engine
from test_gpu_policy_rollout import engine as quad_engine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = L.PF_POLICY_POOL_MAX
# (hidden widths, activation, log_std): two full layers; one narrow ReLU layer; a one-unit first layer; no draw; two odd widths
SHAPES = [((64, 64), "tanh", -0.2), ((7,), "relu", -0.2), ((1, 64), "tanh", -0.2), ((64,), "tanh", None), ((33, 17), "relu", -0.2)]
SENTINEL = 0x7FC12345  # a NaN's bit pattern: what a row without a policy must still hold


def pool(D, A, count=P):
    return [net(D, A, *SHAPES[p % len(SHAPES)][:2], log_std=SHAPES[p % len(SHAPES)][2], seed=20 + p) for p in range(count)]


def make_engine(kind, n):
    eng = quad_engine("hover", n=n) if kind == "hover" else other_engine(kind, n)
    eng.env_reset()
    return eng


def from_counts(counts, n, seed):
    """row_policy with counts[p] rows of policy p, the rest -1, at shuffled places."""
    assert sum(counts) <= n
    rp = torch.full((n,), -1, dtype=torch.int32)
    rp[: sum(counts)] = torch.repeat_interleave(torch.arange(len(counts), dtype=torch.int32), torch.tensor(counts))
    return rp[torch.randperm(n, generator=torch.Generator().manual_seed(seed))].contiguous().to(DEV)


def patterns(n):
    """[(name, row_policy [n] int32)]: explicit assignments whose rows per policy include 0, 1, 63, 64 and 65 where n has room."""
    i = torch.arange(n)
    inter = torch.where(i % 4 >= 2, 1 + i * 16 // n, torch.zeros_like(i)).to(torch.int32)  # lanes 2, 3 of every four: 1 + a segment index
    out = [("interleaved", inter.to(DEV))]
    holes = inter.clone()
    holes[::29] = -1
    holes[n // 2] = 99  # (any value outside 0..P-1 means no policy)
    out.append(("interleaved with holes", holes.to(DEV)))
    if n >= 1000:
        counts = [0, 1, 63, 64, 65, 129, 7, 200, 31, 2, 128, 66, 62, 0, 100, 33, 12]  # 963 rows; 37 without a policy
        assert len(counts) == P and n - sum(counts) == 37
        out.append(("shuffled", from_counts(counts, n, 1)))
    else:
        for c, counts in enumerate(([0] * 16 + [n], [0, 1, n - 1] if n > 1 else [0, 1], [0, 0, n - 1, 0, 0] if n > 1 else [0], [n - 1, 1] if n > 1 else [1])):
            out.append((f"counts {counts}", from_counts(counts + [0] * (P - len(counts)), n, 2 + c)))
    return out


def bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------- 1. rows against the one-policy launch
CASES = [("hover", 1000), ("hover", 1), ("hover", 64), ("hover", 65), ("rocket_quat", 1000), ("dogfight", 1000)]


@pytest.mark.parametrize("kind, n", CASES)
def test_every_row_has_the_bits_of_its_policys_own_launch(kind, n):
    eng = make_engine(kind, n)
    D, A = eng.obs_dim, eng.action_dim
    assert (D, A) == {"hover": (21, 4), "rocket_quat": (30, 7), "dogfight": (123, 6)}[kind]
    assert n == N or kind == "hover"
    pols = pool(D, A)
    obs = eng.obs.clone()
    plans = [(name, rp, eng.policy_pool_plan(rp, P)) for name, rp in patterns(n)]
    for step in (0, 0xFFFFFFFF):
        want_a, want_m = torch.empty(P, n, A, device=DEV), torch.empty(P, n, A, device=DEV)
        for p, pol in enumerate(pols):  # (the reference, once per step index: every policy over all rows)
            eng.policy_act(pol, step_index=step, out=want_a[p], mean_out=want_m[p])
        assert not torch.equal(want_a[0], want_m[0]) and torch.equal(want_a[3], want_m[3])  # (a draw; and entry 3 has none)
        for name, rp, plan in plans:
            assert plan.dtype == torch.uint8 and plan.numel() == L.lib().pf_policy_pool_plan_bytes(n, P)
            a = torch.full((n, A), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
            m = torch.full((n, A), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
            got = eng.policy_act_pool(pols, plan, step_index=step, obs=obs, out=a, mean_out=m)
            assert got[0] is a and got[1] is m
            has = (rp >= 0) & (rp < P)
            pick = rp.clamp(0, P - 1).long().view(1, n, 1).expand(1, n, A)
            ref_a = torch.where(has.view(n, 1), bits(want_a.gather(0, pick)[0]), torch.full_like(bits(a), SENTINEL))
            ref_m = torch.where(has.view(n, 1), bits(want_m.gather(0, pick)[0]), torch.full_like(bits(m), SENTINEL))
            counts = torch.bincount(rp[has].long(), minlength=P).tolist()
            print(f"{kind} n {n} step {step:#x} {name}: rows per policy {counts}, without a policy {int((~has).sum())}")
            assert torch.equal(bits(a), ref_a), (name, step)
            assert torch.equal(bits(m), ref_m), (name, step)
        # without a mean output, into a tensor of the call's own
        a2 = eng.policy_act_pool(pols, plans[0][2], step_index=step, obs=obs)
        assert torch.equal(bits(a2), bits(want_a.gather(0, plans[0][1].long().view(1, n, 1).expand(1, n, A))[0]))
    if n >= 1000:
        counts = torch.bincount(plans[2][1][plans[2][1] >= 0].long(), minlength=P).tolist()
        assert {0, 1, 63, 64, 65} <= set(counts)
    assert torch.equal(eng.obs, obs)
    eng.close()


def test_a_pool_of_one_and_a_plan_built_twice():
    eng = make_engine("hover", 1000)
    pol = net(21, 4, seed=3)
    rp = torch.zeros(1000, dtype=torch.int32, device=DEV)
    plan, again = eng.policy_pool_plan(rp, 1), eng.policy_pool_plan(rp, 1)
    assert torch.equal(plan, again)  # (the plan's bytes are a function of row_policy)
    a, m = eng.policy_act(pol, step_index=7, mean_out=torch.empty(1000, 4, device=DEV))
    b, mb = eng.policy_act_pool([pol], plan, step_index=7, mean_out=torch.empty(1000, 4, device=DEV))
    assert torch.equal(a, b) and torch.equal(m, mb)
    eng.close()


# ---------------------------------------------------------------------------------------------- 2. fp64
def test_means_against_fp64():
    """DESIGN.md section 11's bound on the D = 123 case (two first-layer chunks): the kernel's largest deviation from the float64
    forward is at most 8 x that of torch's own float32 forward, over the same rows -- each row under the policy that flies it."""
    n = 1000
    eng = make_engine("dogfight", n)
    pols = pool(eng.obs_dim, eng.action_dim)
    obs = eng.obs.clone()
    name, rp = patterns(n)[0]
    mean = torch.zeros(n, eng.action_dim, device=DEV)
    eng.policy_act_pool(pols, eng.policy_pool_plan(rp, P), step_index=3, obs=obs, mean_out=mean)
    err = e32 = 0.0
    for p, pol in enumerate(pols):
        rows = rp == p
        if bool(rows.any()):
            ref = pol.forward_reference(obs[rows], dtype=torch.float64)
            err = max(err, (mean[rows].double() - ref).abs().max().item())
            e32 = max(e32, (pol.forward_reference(obs[rows], dtype=torch.float32).double() - ref).abs().max().item())
    print(f"D {eng.obs_dim}, A {eng.action_dim}, {name}: kernel deviation {err:.3e}, torch float32 deviation e32 {e32:.3e}, ratio {err / e32:.2f}")
    assert err <= 8.0 * e32
    eng.close()


# ---------------------------------------------------------------------------------------------- 3. graph capture
def test_the_pool_launch_is_capturable_and_reads_the_weights_at_every_replay():
    n = 1000
    eng = make_engine("rocket_quat", n)
    pols = pool(eng.obs_dim, eng.action_dim, 5)
    rp = patterns(n)[0][1] % 5
    plan = eng.policy_pool_plan(rp, 5)
    obs = eng.obs.clone()
    a, m = torch.zeros(n, 7, device=DEV), torch.zeros(n, 7, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eng.policy_act_pool(pols, plan, step_index=11, obs=obs, out=a, mean_out=m)  # warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # (one call: no parallel branches)
        eng.policy_act_pool(pols, plan, step_index=11, obs=obs, out=a, mean_out=m)
    before = m.clone()
    pols[2].layers[-1][0].mul_(0.5)  # in place: the capture holds the tensors' addresses
    pols[2].layers[-1][1].sub_(0.5)
    pols[4].layers[-1][1].add_(0.25)
    a.zero_(); m.zero_()
    g.replay()
    torch.cuda.synchronize()
    ea, em = eng.policy_act_pool(pols, plan, step_index=11, obs=obs, mean_out=torch.empty_like(m))
    assert torch.equal(a, ea) and torch.equal(m, em)
    changed = (m != before).any(dim=1)
    assert bool(changed[rp == 2].all()) and bool(changed[rp == 4].all()) and not bool(changed[(rp != 2) & (rp != 4)].any())
    eng.close()


# ---------------------------------------------------------------------------------------------- 4. the dogfight's closed loop
NAMES = ("obs", "reward", "terminated", "truncated", "actions", "valid", "mean", "outcome", "outcome_counts")


def test_the_pooled_dogfight_loop_has_the_bits_of_the_unpooled_one():
    kind, k = ("dogfight", 2, 16), 34  # (past the truncation and the resets behind it)
    env, twin = make_env(kind), make_env(kind)
    eng = env.engine
    policy = env_policy(env, seed=5)
    opponents = [env_policy(env, seed=6 + p) for p in range(3)]
    team1 = torch.as_tensor(env.team_flag, device=DEV).repeat(env.num_envs)
    obs0 = eng.obs.clone()
    a = dict(zip(NAMES, (x.clone() for x in env.rollout(policy, k, opponent=opponents, store_mean=True, outcomes=True, pooled=True))))
    b = dict(zip(NAMES, (x.clone() for x in twin.rollout(policy, k, opponent=opponents, store_mean=True, outcomes=True))))
    for name in NAMES:
        if name != "mean":
            assert torch.equal(a[name], b[name]), name
    assert torch.equal(a["mean"][:, ~team1], b["mean"][:, ~team1]) and not torch.equal(a["mean"][:, team1], b["mean"][:, team1])
    assert torch.equal(eng.state, twin.engine.state) and torch.equal(eng.world_done, twin.engine.world_done)
    assert torch.equal(eng.obs, twin.engine.obs) and env._policy_step == twin._policy_step == k
    assert int(a["outcome_counts"][:, 10].sum()) > 0 and bool((a["terminated"] | a["truncated"]).any())  # (copies finished and were reset)
    assert not bool(a["valid"][:, team1].any())
    # on team 1's lanes the mean is the opponent's own, on the observation that step acted on
    group = env._pool_groups[3]
    assert sorted(set(group.tolist())) == [0, 1, 2]
    m = torch.empty(eng.n, eng.action_dim, device=DEV)
    for s in range(k):
        seen = obs0 if s == 0 else a["obs"][s - 1]
        for p, opp in enumerate(opponents):
            eng.policy_act(opp, step_index=s, obs=seen, mean_out=m)
            rows = team1 & (group == p)
            assert torch.equal(a["mean"][s][rows], m[rows]), (s, p)
    env.close(); twin.close()
    # opponent=[p] is opponent=p when pooled, and both are the unpooled run
    one, two, three = make_env(kind), make_env(kind), make_env(kind)
    policy, other = env_policy(one, seed=5), env_policy(one, seed=6)
    x = one.rollout(policy, 20, opponent=other, outcomes=True, pooled=True)
    y = two.rollout(policy, 20, opponent=[other], outcomes=True, pooled=True)
    z = three.rollout(policy, 20, opponent=other, outcomes=True)
    for i, (u, v, w) in enumerate(zip(x, y, z)):
        assert torch.equal(u, v) and torch.equal(u, w), i
    assert torch.equal(one.engine.state, two.engine.state) and torch.equal(one.engine.state, three.engine.state)
    # collect(): the batch of a pooled loop is the unpooled batch but for the mean on team 1's lanes, which no loss reads (never valid)
    ba = one.collect(policy, lambda o: o[:, 0].contiguous(), 12, opponent=other, pooled=True)
    bb = three.collect(policy, lambda o: o[:, 0].contiguous(), 12, opponent=other)
    for key in ("obs", "actions", "values", "advantages", "returns", "valid", "reward", "terminated", "truncated"):
        assert torch.equal(ba[key], bb[key]), key
    valid = ba["valid"]
    assert torch.equal(ba["mean"][valid], bb["mean"][valid]) and torch.equal(ba["logp"][valid], bb["logp"][valid])
    for e in (one, two, three):
        e.close()


# ---------------------------------------------------------------------------------------------- 5. the launch sequence
WORLD_POOL = ["pf_policy_act_pool", "pf_env_step", "pf_world_sync", "pf_env_reset"]


def test_the_pooled_loop_is_one_plan_and_four_launches_per_step():
    env = MAFixedwingDogfightEnv(team_size=2, num_envs=16, seed=11)
    env.reset(seed=11)
    eng = env.engine
    n, W = eng.n, eng.action_dim
    pol = env_policy(env, seed=5)
    opponents = [env_policy(env, seed=6), env_policy(env, seed=7)]
    env._policy_step = STEP0
    out, calls = recorded(eng, lambda: env.rollout(pol, SEQ_K, opponent=opponents, pooled=True))
    assert [c[0] for c in calls] == ["pf_policy_pool_plan"] + WORLD_POOL * SEQ_K, [c[0] for c in calls]
    ctx, row_policy, count, plan, plan_bytes, stream = calls[0][1]
    assert count == 3 and plan_bytes == L.lib().pf_policy_pool_plan_bytes(n, 3)
    acts = [args for name, args in calls if name == "pf_policy_act_pool"]
    for s, (ctx, blocks, count, p, nbytes, a, index, stream) in enumerate(acts):
        assert (count, p, nbytes) == (3, plan, plan_bytes)  # (the one plan, every step)
        assert a == out[4].data_ptr() + 4 * n * W * s and index == (STEP0 + s) & 0xFFFFFFFF, s  # (straight into actions[s]; the index wraps)
    assert eng._opp_act is None  # (no opponent buffer was ever made: nothing is merged)
    assert env._policy_step == (STEP0 + SEQ_K) & 0xFFFFFFFF
    env._policy_step = STEP0
    batch, calls = recorded(eng, lambda: env.collect(pol, lambda o: o[:, 0], SEQ_K, opponent=opponents, pooled=True))
    assert [c[0] for c in calls] == ["pf_policy_pool_plan"] + WORLD_POOL * SEQ_K + ["pf_gae"]
    torch.cuda.synchronize()
    env.close()


# ---------------------------------------------------------------------------------------------- 6. lists of policies on the vector envs
@pytest.mark.parametrize("cls, num_envs, k, kw", [(QuadXHoverVecEnv, 256, 44, dict(max_duration_seconds=1.0, flight_dome_size=1.3)),
                                                  (FixedwingWaypointsVecEnv, 64, 34, dict(max_duration_seconds=1.0, flight_dome_size=24.5))],
                         ids=["quadx_hover", "fixedwing_waypoints"])
def test_a_list_of_policies_is_the_hand_written_loop(cls, num_envs, k, kw):
    """Four policies on contiguous quarters of the envs (the default group), k past the time limit (40 steps at 40 Hz, 30 at 30 Hz):
    against per step four policy_act calls merged by group, then env_step; the outcome counts against episode_outcomes on that loop."""
    env, twin = (cls(num_envs, seed=3, autoreset_mode="next_step", **kw) for _ in range(2))
    env.reset(seed=3); twin.reset(seed=3)
    eng = twin.engine
    n, D, A = num_envs, eng.obs_dim, eng.action_dim
    pols = [net(D, A, *SHAPES[g][:2], log_std=SHAPES[g][2], seed=40 + g) for g in (0, 1, 3, 4)]
    group = torch.arange(n, device=DEV, dtype=torch.int32) // (n // 4)
    want = dict(obs=torch.empty(k, n, D, device=DEV), reward=torch.empty(k, n, device=DEV), terminated=torch.empty(k, n, dtype=torch.bool, device=DEV),
                truncated=torch.empty(k, n, dtype=torch.bool, device=DEV), actions=torch.empty(k, n, A, device=DEV), mean=torch.empty(k, n, A, device=DEV))
    counts = torch.zeros(4, 16, dtype=torch.int64, device=DEV)
    outcome = torch.zeros(k, n, dtype=torch.uint8, device=DEV)
    each_a, each_m = torch.empty(4, n, A, device=DEV), torch.empty(4, n, A, device=DEV)
    pick = group.long().view(1, n, 1).expand(1, n, A)
    for s in range(k):
        for g, pol in enumerate(pols):
            eng.policy_act(pol, step_index=s, out=each_a[g], mean_out=each_m[g])
        want["actions"][s], want["mean"][s] = each_a.gather(0, pick)[0], each_m.gather(0, pick)[0]
        o, r, te, tr = eng.env_step(want["actions"][s])
        want["obs"][s], want["reward"][s], want["terminated"][s], want["truncated"][s] = o, r, te, tr
        eng.episode_outcomes(te, tr, counts, group=group, n_groups=4, outcome_out=outcome[s])
    out = env.rollout(pols, k, store_mean=True, outcomes=True)
    assert len(out) == 9
    got = dict(zip(("obs", "reward", "terminated", "truncated", "actions", "mean", "outcome", "outcome_counts"), out))
    for key, v in want.items():
        assert torch.equal(got[key], v), key
    assert torch.equal(env.engine.state, eng.state)
    ends = (want["terminated"] | want["truncated"]).sum(0)
    assert int(ends.min()) >= 1  # (every env crosses an episode end and its reset)
    assert tuple(got["outcome_counts"].shape) == (4, 16) and torch.equal(got["outcome_counts"], counts) and torch.equal(got["outcome"], outcome)
    assert int(counts[:, 0].min()) >= n // 4
    rows = env.episode_outcomes_dict()
    assert len(rows) == 4 and [r["episodes"] for r in rows] == counts[:, 0].tolist()
    assert not torch.equal(each_a[0], each_a[1])  # (the policies differ: a merge by the wrong group would show)
    # an explicit group, and a list of one against the policy itself
    flipped = (3 - group).contiguous()
    env.reset(seed=3); twin.reset(seed=3)
    x = env.rollout(pols, 6, group=flipped)
    for g, pol in enumerate(pols):
        eng.policy_act(pol, step_index=0, out=each_a[g])
    assert torch.equal(x[4][0], each_a.gather(0, flipped.long().view(1, n, 1).expand(1, n, A))[0])
    env.reset(seed=3); twin.reset(seed=3)
    x, y = env.rollout([pols[0]], 6, store_mean=True), twin.rollout(pols[0], 6, store_mean=True, fused=False)
    for u, v in zip(x[:6], y[:6]):
        assert torch.equal(u, v)
    env.close(); twin.close()


# ---------------------------------------------------------------------------------------------- 7. the example
def test_example_17_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "17_checkpoint_tournament.py"), "256", "48"], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [l for l in out.stdout.splitlines() if l.startswith("policy ")]
    assert len(rows) == 4, out.stdout
    assert all("episodes" in l for l in rows)

"""Rocket-Landing on the device (env_kernel<Rocket, PF_TASK_ROCKET_LANDING, kRuntimeMode>, pyflyt_amd/csrc/rocket_landing.hpp):
the reference's own RocketLandingEnv recorded on the fp64 pad model (tests/golden/gen_rocket_landing.py) replayed through
PF_NOISE_INJECT -- 70 lanes in phase with host resets and through both in-kernel auto-resets, then 70 lanes out of phase over five
recordings at once (tests/rocket_lane_programs.py) --, the Philox draws against the oracle's generator, device known-answer tests
at 4 096 lanes, rollout / lane-offset bit identity, the action sampler."""
from __future__ import annotations

import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 70  # (a ragged second wave)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# the env fixtures' bounds (tests/test_gpu_golden.py): 1e-4 relative per observation vector, 1e-3 on an observation that carries a
# contact impulse -- here the steps with the rocket's legs within reach of the pad or the floor (base z below 2.7 m), where the
# contact solve runs every tick. Measured on the MI355X (each replay prints its worst): 2.5e-5 over the flights (euler; random
# 1.3e-5, land 1.9e-6), 2.1e-5 on the contact steps (offpad / hard 1.1e-7, land 8.1e-7).
# The four fixtures for the branches the first five do not reach (flight / contact steps): timeout 6.7e-7 / -, ceiling 2.7e-7 / -,
# lateral 8.6e-7 / -, rest_tilt 7.2e-8 on its reset observations and 1.8e-4 on its 80 steps, every one of them a pad contact (set down tilted
# and yawed, the rocket settles through the contact solve on every tick) -- inside RTOL_IMPACT as recorded, so no gentler pose was
# needed.
# The three auto-reset modes (off / next_step / same_step) give the same worst errors to the digits above on all nine fixtures:
# the in-kernel resets run the host reset's code on the same inputs; terminal observations in final_obs: at most 2.1e-5 (euler),
# 1.8e-4 (rest_tilt). Step and event counters matched the host's bookkeeping on every call.
# The mixed run (70 lanes out of phase over offpad / land / hard / rest_tilt / ceiling, 371 and 370 calls, 23 555 and 24 522
# compared lane-calls in mode off / same_step): flight 1.9e-6, contact 1.8e-4, reset observations 8.1e-8, rewards 6.8e-6 -- each the
# worst of the five recordings run alone, and bit for bit their outputs: 0 lane-call outputs differ in any bit, in both modes.
# Philox against inject fed the host's draws (62 events x 130 lanes, 260 NEXT_STEP resets, a masked reset): observations 3.6e-7,
# rewards 1.9e-5; the negative controls miss RTOL by 19 746x (counter off by one), 356x (streams 0 and 1 swapped: the smallest) and
# 19 509x (lane keyed without lane_offset).
RTOL = 1e-4
RTOL_IMPACT = 1e-3
Z_CONTACT = 2.7
LOW = np.array([-1.0, -1.0, -1.0, 0.0, 0.0, -1.0, -1.0], dtype=np.float32)
FIXTURES = ("random", "euler", "offpad", "land", "hard", "timeout", "ceiling", "lateral", "rest_tilt")


def load(name):
    return np.load(os.path.join(GOLD, f"env_rocket_landing_{name}.npz"))


def dev_cols(a, n=N):
    a = np.nan_to_num(np.asarray(a, dtype=np.float64))
    return torch.tensor(np.repeat(a[:, None], n, axis=1), dtype=torch.float32, device=DEV).contiguous()


def obs_groups(quat):
    g, k = [], 0
    for w in (3, 4 if quat else 3, 3, 3, 7, 9, 1):
        g.append((k, k + w))
        k += w
    return g


def vec_err(got, ref, groups):
    e = 0.0
    for lo, hi in groups:
        scale = max(1.0, float(np.linalg.norm(ref[lo:hi])))
        e = max(e, float(np.abs(got[:, lo:hi] - ref[lo:hi]).max()) / scale)
    return e


def fixture_params(g, **kw):
    from pyflyt_amd import _lib as L
    from pyflyt_amd import build_params

    opts = int(g["options"])
    kw.setdefault("autoreset", "off")
    if "max_duration_seconds" in g.files:  # (stored where the recording set one: gen_rocket_landing.py)
        kw.setdefault("max_duration_seconds", float(g["max_duration_seconds"]))
    return build_params("rocket", "rocket_landing", noise="inject", ceiling=float(g["ceiling"]),
                        max_displacement=float(g["max_displacement"]), angle_representation="quaternion" if int(g["angle_repr"]) else "euler",
                        sparse_reward=bool(g["sparse"]), reset_options=(L.RL_RANDOMIZE_DROP | L.RL_ACCELERATE_DROP) if opts < 0 else opts,
                        start_pos=g["start_pos"], start_orn=g["start_orn"], **kw)


POISON = 1.0e6  # the action handed to a NEXT_STEP reset call: large, finite, outside every box


def replay(name, corrupt=None, autoreset="off"):
    """corrupt = (step, lane, group, word, delta): one word of the device state moved before that step (the negative test).
    autoreset: "off" -- every reset is an env_reset from the host; "next_step" -- the env_step call after a terminal step IS the reset
    (reward 0, not done, whatever its action); "same_step" -- the terminal call carries the reset's inputs, the terminal observation
    and info go to final_obs / final_info, obs is the reset's. In both in-kernel modes the lane's step counter and event counter
    (eng.ints()) are checked against the host's bookkeeping on every call."""
    from pyflyt_amd import _lib as L
    from pyflyt_amd.engine import BatchEngine

    g = load(name)
    P = fixture_params(g, autoreset=autoreset)
    eng = BatchEngine(P, N, device=DEV)
    D = eng.obs_dim
    assert D == g["obs"].shape[1] and eng.groups == 9
    G = obs_groups(bool(P.angle_repr))
    zi = 12 if P.angle_repr else 11
    resets = set(int(k) for k in g["reset_before"])
    ri, worst, worst_impact, worst_final = 0, 0.0, 0.0, 0.0
    seen = dict(term=0, trunc=0, complete=0)
    steps, events = 0, 0  # the host's copy of the lane's step counter and event counter
    zero_xr = torch.zeros(eng.settle_ticks, N, dtype=torch.float32, device=DEV)
    zero_u = torch.zeros(6, N, dtype=torch.float32, device=DEV)

    def check_counters(where):
        if autoreset != "off":
            c = eng.ints().cpu().numpy()
            assert (c[:, 0] == steps).all() and (c[:, 2] == events).all(), (name, where, c[0], steps, events)

    def check_reset_obs(obs, where):
        nonlocal ri, worst
        e = vec_err(obs.double().cpu().numpy(), g["reset_obs"][ri], G)
        assert e < RTOL, (name, "reset", where, ri, e)
        worst = max(worst, e)
        ri += 1

    def do_reset():
        nonlocal steps, events
        check_reset_obs(eng.env_reset(xi_reset=dev_cols(g["reset_xi"][ri]), u_targets=dev_cols(g["reset_u"][ri])), "host")
        steps, events = 0, events + 1
        check_counters("host reset")

    def next_step_reset(k):
        """the call after a terminal step: once with a poisoned action (and step draws), once -- from the same state -- with zeros;
        nothing may differ"""
        nonlocal steps, events
        before = eng.state.clone()
        outs = []
        for fill in (POISON, 0.0):
            eng.state.copy_(before)
            a = torch.full((N, 7), fill, dtype=torch.float32, device=DEV)
            xi = torch.full((eng.ticks_per_step, N), fill, dtype=torch.float32, device=DEV)
            obs, rew, term, trunc = eng.env_step(a, xi=xi, xi_reset=dev_cols(g["reset_xi"][ri]), u_targets=dev_cols(g["reset_u"][ri]))
            outs.append((eng.state.clone(), obs.clone(), rew.clone(), term.clone(), trunc.clone()))
        assert all(torch.equal(x, y) for x, y in zip(*outs)), (name, k, "the action of a reset call changed something")
        assert float(rew.abs().max()) == 0.0 and not bool(term.any()) and not bool(trunc.any()), (name, k)
        assert not (eng.flags().cpu().numpy() & ~L.F_CONTACT).any(), (name, k)
        check_reset_obs(obs, "next_step")
        steps, events = 0, events + 1
        check_counters("next_step reset")

    do_reset()
    for k in range(len(g["action"])):
        if k in resets:
            if autoreset == "off":
                do_reset()
            elif autoreset == "next_step":
                next_step_reset(k)
        a = torch.tensor(np.repeat(g["action"][k][None], N, axis=0), dtype=torch.float32, device=DEV).contiguous()
        if corrupt is not None and corrupt[0] == k:
            eng.state[corrupt[2], corrupt[1], corrupt[3]] += corrupt[4]
        same = autoreset == "same_step" and (k + 1) in resets  # this call ends the episode and restarts it
        if autoreset == "off":
            obs, rew, term, trunc = eng.env_step(a, xi=dev_cols(g["xi"][k]))
        else:  # (the reset inputs are always there: a lane that ended where the recording did not must fail an assertion, not read a null pointer)
            obs, rew, term, trunc = eng.env_step(a, xi=dev_cols(g["xi"][k]), xi_reset=dev_cols(g["reset_xi"][ri]) if same else zero_xr,
                                                 u_targets=dev_cols(g["reset_u"][ri]) if same else zero_u)
        impact = bool(g["info_col"][k]) or g["obs"][k][zi] < Z_CONTACT or (k > 0 and g["obs"][k - 1][zi] < Z_CONTACT)
        assert bool(g["term"][k] or g["trunc"][k]) == ((k + 1) in resets or (k + 1 == len(g["action"]) and bool(g["term"][k] or g["trunc"][k])))
        step_obs = eng.final_obs if same else obs
        e = vec_err(step_obs.double().cpu().numpy(), g["obs"][k], G)
        if impact:
            assert e < RTOL_IMPACT, (name, k, e)
            worst_impact = max(worst_impact, e)
        else:
            assert e < RTOL, (name, k, e)
            worst = max(worst, e)
        if same:
            worst_final = max(worst_final, e)
        r = rew.double().cpu().numpy()
        assert np.abs(r - g["reward"][k]).max() <= 1e-3 * max(1.0, abs(g["reward"][k])), (name, k, r[0], g["reward"][k])
        assert (term.cpu().numpy() == bool(g["term"][k])).all() and (trunc.cpu().numpy() == bool(g["trunc"][k])).all(), (name, k)
        f = (eng.final_info[:, 0] if same else eng.flags()).cpu().numpy()
        assert (((f & L.F_INFO_OOB) != 0) == bool(g["info_oob"][k])).all(), (name, k)
        assert (((f & L.F_INFO_COLLISION) != 0) == bool(g["info_col"][k])).all(), (name, k)
        assert (((f & L.F_INFO_COMPLETE) != 0) == bool(g["info_complete"][k])).all() and not (f & L.F_NONFINITE).any(), (name, k)
        steps, events = steps + 1, events + 1
        if same:  # final_info: the done bits of the episode that ended; the live flags: those of the one that began
            assert (((f & L.F_TERMINATED) != 0) == bool(g["term"][k])).all() and (((f & L.F_TRUNCATED) != 0) == bool(g["trunc"][k])).all(), (name, k)
            assert not (eng.flags().cpu().numpy() & ~L.F_CONTACT).any(), (name, k)
            check_reset_obs(obs, "same_step")
            steps, events = 0, events + 1
        check_counters(k)
        seen["term"] += int(g["term"][k])
        seen["trunc"] += int(g["trunc"][k])
        seen["complete"] += int(g["info_complete"][k] and g["trunc"][k])
    assert ri == len(g["reset_obs"])
    print(f"{name} [{autoreset}]: worst {worst:.2e} over {len(g['action'])} steps, {ri} resets, ended {seen}; worst observation with a contact in it "
          f"{worst_impact:.2e}" + (f"; worst terminal observation in final_obs {worst_final:.2e}" if autoreset == "same_step" else ""))
    return seen


@pytest.mark.parametrize("autoreset", ["off", "next_step", "same_step"])
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_replay(name, autoreset):
    seen = replay(name, autoreset=autoreset)
    if name in ("land", "rest_tilt"):  # the resting velocity got under 0.02 on the device: env_complete
        assert seen["complete"] >= (4 if name == "rest_tilt" else 1)
    if name in ("random", "offpad", "hard", "ceiling", "lateral"):
        assert seen["term"] >= 1
    if name == "timeout":
        assert seen["trunc"] == 2 and seen["term"] == 0


def test_replay_catches_a_corrupted_state_word():
    """one word of the state (the rocket's z velocity, lane 5) moved by 1e-3 m/s mid-flight: the replay must fail"""
    with pytest.raises(AssertionError):
        replay("land", corrupt=(40, 5, 2, 2, 1e-3))


# ------------------------------------------------------------------ mixed waves (tests/rocket_lane_programs.py)
def _mixed_engine(mode):
    from pyflyt_amd import _lib as L
    from pyflyt_amd import build_params
    from pyflyt_amd.engine import BatchEngine

    P = build_params("rocket", "rocket_landing", noise="inject", autoreset=mode, ceiling=20.0, angle_representation="quaternion",
                     sparse_reward=False, reset_options=L.RL_RANDOMIZE_DROP)
    return BatchEngine(P, N, device=DEV)


def run_schedule(S, A, mode):
    """One call per row of the schedule: a step launch for every lane, then a masked env_reset for the lanes whose op is no STEP.
    Everything the calls return is kept on the device and read once: obs / reward / term / trunc / flags [calls, n, ...] (of a
    RESET op: the reset launch's), and final_obs / final_info under same_step."""
    eng = _mixed_engine(mode)
    T, n = S["kind"].shape
    assert n == N and eng.obs_dim == A["ref_obs"].shape[2]
    up = lambda x: torch.tensor(x, device=DEV).contiguous()  # noqa: E731
    act, xi, xr, u, mask = up(A["actions"]), up(A["xi"]), up(A["xi_reset"]), up(A["u_targets"]), up(A["reset_mask"])
    any_reset = A["reset_mask"].any(1)
    out = dict(obs=torch.zeros(T, n, eng.obs_dim, device=DEV), reward=torch.zeros(T, n, device=DEV), term=torch.zeros(T, n, dtype=torch.bool, device=DEV),
               trunc=torch.zeros(T, n, dtype=torch.bool, device=DEV), flags=torch.zeros(T, n, dtype=torch.int32, device=DEV))
    if mode == "same_step":
        out.update(final_obs=torch.zeros(T, n, eng.obs_dim, device=DEV), final_info=torch.zeros(T, n, dtype=torch.int32, device=DEV))
    eng.env_reset(xi_reset=torch.zeros(eng.settle_ticks, n, device=DEV), u_targets=u)  # (a defined state for the delays to idle in)
    for t in range(T):
        if mode == "same_step":
            eng.env_step(act[t], xi=xi[t], xi_reset=xr[t], u_targets=u)
            out["final_obs"][t].copy_(eng.final_obs)
            out["final_info"][t].copy_(eng.final_info[:, 0])
        else:
            eng.env_step(act[t], xi=xi[t])
        for key, src in (("obs", eng.obs), ("reward", eng.reward), ("term", eng.terminated), ("trunc", eng.truncated), ("flags", eng.flags())):
            out[key][t].copy_(src)
        if any_reset[t]:
            eng.env_reset(mask=mask[t], xi_reset=xr[t], u_targets=u)
            out["obs"][t][mask[t]] = eng.obs[mask[t]]
            out["flags"][t][mask[t]] = eng.flags()[mask[t]]
    return {k: v.cpu().numpy() for k, v in out.items()}


def group_err(got, ref, groups):
    """vec_err for [.., D] arrays: per row, the worst group error relative to max(1, |the reference's group|)"""
    e = np.zeros(got.shape[:-1])
    for lo, hi in groups:
        scale = np.maximum(1.0, np.linalg.norm(ref[..., lo:hi], axis=-1))
        e = np.maximum(e, np.abs(got[..., lo:hi].astype(np.float64) - ref[..., lo:hi]).max(-1) / scale)
    return e


def check_schedule(S, A, out, label):
    """every compared lane-call of a schedule run against its lane's recording at the lane's own cursor, under replay's bounds"""
    import rocket_lane_programs as RLP
    from pyflyt_amd import _lib as L

    G = obs_groups(True)
    step, reset = S["kind"] == RLP.STEP, S["kind"] == RLP.RESET
    same = step & (S["ri"] >= 0)  # reset by the kernel inside a step call: the step's observation is in final_obs
    e_obs = group_err(out["obs"], A["ref_obs"], G)
    e_step = np.where(same, group_err(out["final_obs"], A["ref_final"], G), e_obs) if same.any() else e_obs
    flight, impact = step & ~A["impact"], step & A["impact"]
    bad = (flight & ~(e_step < RTOL)) | (impact & ~(e_step < RTOL_IMPACT)) | ((reset | same) & ~(e_obs < RTOL))
    assert not bad.any(), (label, "first failing (call, lane)", np.argwhere(bad)[:5].tolist(), e_step[bad][:5], e_obs[bad][:5])
    e_rew = np.abs(out["reward"] - A["ref_reward"]) / np.maximum(1.0, np.abs(A["ref_reward"]))
    assert (e_rew[step] <= 1e-3).all(), (label, np.argwhere(step & (e_rew > 1e-3))[:5].tolist())
    assert (out["term"][step] == A["ref_term"][step]).all() and (out["trunc"][step] == A["ref_trunc"][step]).all(), label
    info = np.where(same, out["final_info"], out["flags"]) if same.any() else out["flags"]
    bits = L.F_INFO_OOB | L.F_INFO_COLLISION | L.F_INFO_COMPLETE | L.F_NONFINITE
    assert ((info & bits)[step] == A["ref_info"][step]).all(), (label, np.argwhere(step & ((info & bits) != A["ref_info"]))[:5].tolist())
    if same.any():
        done = np.where(A["ref_term"], L.F_TERMINATED, 0) | np.where(A["ref_trunc"], L.F_TRUNCATED, 0)
        assert ((out["final_info"] & (L.F_TERMINATED | L.F_TRUNCATED))[same] == done[same]).all(), label
    assert not (out["flags"][reset | same] & ~L.F_CONTACT).any(), label
    n_cmp = int(step.sum() + reset.sum() + same.sum())
    w = lambda m: float(e_step[m].max()) if m.any() else 0.0  # noqa: E731
    print(f"{label}: {n_cmp} compared lane-calls over {S['kind'].shape[0]} calls; worst in flight {w(flight):.2e}, with a contact {w(impact):.2e}, "
          f"reset observations {float(e_obs[reset | same].max()):.2e}, rewards {float(e_rew[step].max()):.2e}")
    return n_cmp


_SOLO = {}


def solo_run(name, mode):
    """one fixture alone through the mixed run's route (randomize-drop, the pose in u_targets): 70 lanes in phase, one pass"""
    import rocket_lane_programs as RLP

    if (name, mode) not in _SOLO:
        fx = [RLP.load(name)]
        S = RLP.schedule(fx, mode, delays=np.zeros(N, dtype=np.int64))
        A = RLP.assemble(S, fx)
        out = run_schedule(S, A, mode)
        check_schedule(S, A, out, f"{name} alone [{mode}]")
        for key, v in out.items():  # lanes in phase are bit-identical
            assert (v.view(np.uint8).reshape(v.shape[0], N, -1) == v.view(np.uint8).reshape(v.shape[0], N, -1)[:, :1]).all(), (name, mode, key)
        _SOLO[(name, mode)] = {key: v[:, 0] for key, v in out.items()}
    return _SOLO[(name, mode)]


@pytest.mark.parametrize("mode", ["off", "same_step"])
def test_mixed_wave_replay(mode):
    """70 lanes, five recordings, every lane out of phase with every other (tests/rocket_lane_programs.py): each lane against its own
    recording at its own cursor while its wave-mates are in the pad solve, on the floor, in flight, being reset, done or idle.
    mode "off": masked env_reset from the host; "same_step": the kernel resets a lane inside a step call that its wave-mates
    step through. Then the same lanes against each recording run ALONE through the same route: a wave-mate changes no bit."""
    import rocket_lane_programs as RLP

    fixtures = [RLP.load(n) for n in RLP.MIXED_FIXTURES]
    S = RLP.schedule(fixtures, mode)
    A = RLP.assemble(S, fixtures)
    out = run_schedule(S, A, mode)
    n_cmp = check_schedule(S, A, out, f"mixed [{mode}]")
    assert n_cmp == int((S["kind"] != RLP.IDLE).sum() + ((S["kind"] == RLP.STEP) & (S["ri"] >= 0)).sum())  # no compared lane-call left out
    T = S["kind"].shape[0]
    differing = 0
    for i in range(N):
        fi, d = int(S["fix"][i]), int(S["delays"][i])
        solo = solo_run(RLP.MIXED_FIXTURES[fi], mode)
        rows = np.arange(d, T)
        src = (rows - d) % int(S["period"][fi])
        stepped = S["kind"][rows, i] == RLP.STEP  # (a RESET op's step launch runs on whatever the lane was left in: not compared)
        ends = S["ri"][rows, i] >= 0
        for key in out:
            sel = stepped if key in ("reward", "term", "trunc") else ((stepped & ends) if key.startswith("final") else np.ones(len(rows), bool))
            a, b = out[key][rows, i][sel], solo[key][src][sel]
            if len(a) == 0:
                continue
            differing += int((a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(1).sum())
    print(f"mixed [{mode}] against each recording alone: {differing} lane-call outputs differ in some bit")
    assert differing == 0


# ------------------------------------------------------------------ the Philox draws (Noise, uav_vehicles.hpp)
PH_SEED, PH_OFFSET, PH_N, PH_STEPS, PH_MASKED_AT, PH_MASKED = 0x5EED0000BEEF, 4099, 130, 60, 30, (3, 64, 65, 129)


def _philox_engine(noise):
    from pyflyt_amd import build_params
    from pyflyt_amd.engine import BatchEngine

    # default reset options (a randomized drop at -100 m/s), ceiling 500; half-second episodes, so that every lane is truncated
    # and restarted by the kernel twice within the run
    P = build_params("rocket", "rocket_landing", noise=noise, autoreset="next_step", seed=PH_SEED, max_duration_seconds=0.5)
    return BatchEngine(P, PH_N, device=DEV, lane_offset=PH_OFFSET)


def host_draws(P, ev, mistake=None):
    """What PF_NOISE_PHILOX draws for an event of every lane, from the oracle's generator and the keys Noise documents:
    Philox4x32(seed; global lane, event counter, call, stream) with call = flat >> 3 for the eight normals of a call and flat >> 2 for
    the four uniforms; stream 0 = a step's booster draws (n_motors + z, one per physics tick), stream 1 = a reset's settle draws,
    stream 2 = the six spawn uniforms, each mapped into its box lo + (hi - lo) u (begin_reset: x, y in +-0.1 max_displacement, z in
    0.8-0.9 ceiling, roll / pitch / yaw in +-0.3). Returns xi [6, n], xi_reset [20, n], u_targets [6, n] in float32.
    mistake: "counter" (event counter off by one), "streams" (0 and 1 swapped), "lane" (keyed without lane_offset)."""
    import ctypes as C

    from oracle import oracle as O

    lib = O.lib()
    lib.orc_normal8.argtypes = [C.c_uint64] + [C.c_uint32] * 4 + [C.POINTER(C.c_double)]
    z8, u4 = (C.c_double * 8)(), (C.c_double * 4)()
    s_step, s_settle = (1, 0) if mistake == "streams" else (0, 1)
    xi, xr, ut = np.zeros((6, PH_N)), np.zeros((20, PH_N)), np.zeros((6, PH_N))
    s = 0.1 * float(P.max_displacement)
    lo = np.array([-s, -s, 0.8 * float(P.ceiling), -0.3, -0.3, -0.3])
    hi = np.array([s, s, 0.9 * float(P.ceiling), 0.3, 0.3, 0.3])
    for i in range(PH_N):
        lane = i if mistake == "lane" else PH_OFFSET + i
        ctr = int(ev[i]) + (1 if mistake == "counter" else 0)
        lib.orc_normal8(PH_SEED, lane, ctr, 0, s_step, z8)
        xi[:, i] = np.array(z8[:6]) + P.n_motors
        for call in range(3):
            lib.orc_normal8(PH_SEED, lane, ctr, call, s_settle, z8)
            m = min(8, 20 - 8 * call)
            xr[8 * call:8 * call + m, i] = np.array(z8[:m]) + P.n_motors
        for call in range(2):
            lib.orc_uniform4(PH_SEED, lane, ctr, call, 2, u4)
            for j in range(4 * call, min(6, 4 * call + 4)):
                ut[j, i] = lo[j] + (hi[j] - lo[j]) * u4[j - 4 * call]
    dev = lambda x: torch.tensor(x, dtype=torch.float32, device=DEV).contiguous()  # noqa: E731
    return dev(xi), dev(xr), dev(ut)


def _philox_run(noise, actions=None, mistake=None):
    """PH_STEPS calls with pf_sample_actions' actions, a masked reset of a few lanes midway (their event counters run ahead from
    there). The inject context is fed host_draws for the event counter the HOST predicts: one event per call and lane, whatever the
    call does to the lane (a step or the kernel's NEXT_STEP reset), one more for a masked reset."""
    eng = _philox_engine(noise)
    inject = noise == "inject"
    P = eng.params
    ev = np.zeros(PH_N, dtype=np.int64)
    mask = torch.zeros(PH_N, dtype=torch.bool, device=DEV)
    mask[list(PH_MASKED)] = True
    rec = dict(obs=[], reward=[], term=[], trunc=[], flags=[], ctr=[], actions=[])

    def keep(step_outputs):
        rec["obs"].append(eng.obs.cpu().numpy().astype(np.float64))
        c = eng.ints().cpu().numpy()
        rec["flags"].append(c[:, 1].copy())
        rec["ctr"].append(c[:, 2].copy())
        rec["reward"].append(eng.reward.cpu().numpy().astype(np.float64) if step_outputs else np.zeros(PH_N))
        rec["term"].append(eng.terminated.cpu().numpy().copy() if step_outputs else np.zeros(PH_N, bool))
        rec["trunc"].append(eng.truncated.cpu().numpy().copy() if step_outputs else np.zeros(PH_N, bool))

    def reset(m):
        if inject:
            _, xr, ut = host_draws(P, ev, mistake)
            eng.env_reset(mask=m, xi_reset=xr, u_targets=ut)
        else:
            eng.env_reset(mask=m)
        ev[:] += 1 if m is None else m.cpu().numpy()
        keep(False)

    reset(None)
    for k in range(PH_STEPS):
        if k == PH_MASKED_AT:
            reset(mask)
        if actions is None:
            a = torch.empty(PH_N, 7, dtype=torch.float32, device=DEV)
            eng.sample_actions(a, k)
            rec["actions"].append(a)
        else:
            a = actions[k]
        if inject:
            xi, xr, ut = host_draws(P, ev, mistake)
            eng.env_step(a, xi=xi, xi_reset=xr, u_targets=ut)
        else:
            eng.env_step(a)
        ev += 1
        keep(True)
        if mistake is None:
            assert (rec["ctr"][-1] == ev).all(), (noise, k, rec["ctr"][-1][:4], ev[:4])  # the host's prediction of the event counter
    return {key: (v if key == "actions" else np.stack(v)) for key, v in rec.items()}


def test_philox_equals_inject_fed_the_documented_draws():
    """The Philox context against an inject context that is handed, from the host, the draws Noise documents (host_draws): the same
    observations (RTOL per vector; the auxiliary group carries the noisy throttle), rewards and flags, through the kernel's
    NEXT_STEP resets and a masked reset. Three controls, each with ONE mistake in the host's keys, must each miss the bound by at
    least 10x somewhere: the comparison can see an off-by-one counter, swapped streams and a lane keyed without its offset."""
    from pyflyt_amd import _lib as L

    G = obs_groups(True)
    ph = _philox_run("philox")
    inj = _philox_run("inject", actions=ph["actions"])
    e = group_err(inj["obs"], ph["obs"], G)
    e_rew = np.abs(inj["reward"] - ph["reward"]) / np.maximum(1.0, np.abs(ph["reward"]))
    restarts = int((ph["term"] | ph["trunc"]).sum())
    print(f"philox vs inject fed the host's draws: {e.shape[0]} events x {PH_N} lanes, {restarts} NEXT_STEP resets; worst observation {e.max():.2e}, "
          f"reward {e_rew.max():.2e}")
    assert e.max() < RTOL, np.unravel_index(e.argmax(), e.shape)
    assert e_rew.max() <= 1e-3
    assert (inj["term"] == ph["term"]).all() and (inj["trunc"] == ph["trunc"]).all() and (inj["flags"] == ph["flags"]).all()
    assert (inj["ctr"] == ph["ctr"]).all() and not (ph["flags"] & L.F_NONFINITE).any()
    assert restarts >= 2 * PH_N and len(set(ph["ctr"][-1].tolist())) == 2  # every lane restarted twice; the masked lanes run one event ahead
    ratios = {}
    for mistake in ("counter", "streams", "lane"):
        bad = _philox_run("inject", actions=ph["actions"], mistake=mistake)
        ratios[mistake] = float(group_err(bad["obs"], ph["obs"], G).max()) / RTOL
    print("negative controls, worst observation error over the bound: " + ", ".join(f"{k} {v:.1f}x" for k, v in ratios.items()))
    assert min(ratios.values()) >= 10.0, ratios


# ------------------------------------------------------------------ device known-answer tests (4 096 lanes)
def _run_until_done(env, steps):
    zero = torch.zeros(env.num_envs, 7, dtype=torch.float32, device=DEV)
    done = torch.zeros(env.num_envs, dtype=torch.bool, device=DEV)
    for _ in range(steps):
        _, _, te, tr, info = env.step(zero)
        done |= te | tr
        if bool(done.all()):
            break
    return done, info.materialize()


def test_kat_rest_on_pad_completes():
    from pyflyt_amd.gym_envs import RocketLandingVecEnv

    env = RocketLandingVecEnv(4096, ceiling=20.0, start_pos=(0.3, -0.4, 2.60), autoreset_mode="disabled", seed=1)
    obs, _ = env.reset(options={})
    assert obs.shape == (4096, 30) and float(obs[:, -1].abs().max()) == 0.0  # the pad bit lags: 0 after a reset
    done, info = _run_until_done(env, 400)
    assert bool(done.all()) and bool(info["env_complete"].all()) and not bool(info["fatal_collision"].any())
    z = env.engine.state[0, :, 2]
    assert float((z - 2.575).abs().max()) < 2e-3
    env.close()


def test_kat_floor_beside_pad_is_fatal():
    from pyflyt_amd.gym_envs import RocketLandingVecEnv

    env = RocketLandingVecEnv(4096, ceiling=20.0, start_pos=(4.0, 1.0, 3.0), autoreset_mode="disabled", seed=2)
    env.reset(options={})
    done, info = _run_until_done(env, 100)
    assert bool(done.all()) and bool(info["fatal_collision"].all()) and not bool(info["env_complete"].any())
    env.close()


def test_kat_out_of_bounds():
    from pyflyt_amd.gym_envs import RocketLandingVecEnv

    env = RocketLandingVecEnv(4096, ceiling=20.0, max_displacement=1.0, start_pos=(1.5, 0.0, 10.0), autoreset_mode="disabled", seed=3)
    env.reset(options={})
    done, info = _run_until_done(env, 2)
    assert bool(done.all()) and bool(info["out_of_bounds"].all()) and not bool(info["fatal_collision"].any())
    env.close()


# ------------------------------------------------------------------ bit identity
def _engine(n, lane_offset=0, autoreset="next_step", ceiling=20.0):
    from pyflyt_amd import build_params
    from pyflyt_amd.engine import BatchEngine

    P = build_params("rocket", "rocket_landing", noise="philox", autoreset=autoreset, seed=7, ceiling=ceiling)
    return BatchEngine(P, n, device=DEV, lane_offset=lane_offset)


def test_rollout_matches_single_steps():
    """rollout(k) == k x (sample_actions + env_step), bit for bit, across auto-resets (randomized drops at 100 m/s from 16-18 m)"""
    n, k = 200, 60
    a, b = _engine(n), _engine(n)
    a.env_reset()
    b.env_reset()
    obs, rew, term, trunc, acts = a.rollout(k, step_index0=5)
    out = torch.empty(n, 7, dtype=torch.float32, device=DEV)
    ends = 0
    for s in range(k):
        b.sample_actions(out, 5 + s)
        assert torch.equal(out, acts[s])
        o, r, te, tr = b.env_step(out)
        assert torch.equal(o, obs[s]) and torch.equal(r, rew[s]) and torch.equal(te, term[s]) and torch.equal(tr, trunc[s]), s
        ends += int((te | tr).sum())
    assert ends > n  # every lane restarted at least once on average
    assert torch.equal(a.state, b.state)


def test_lane_matches_lane_offset():
    n, k = 130, 40
    big = _engine(n)
    big.env_reset()
    out = torch.empty(n, 7, dtype=torch.float32, device=DEV)
    traj = []
    for s in range(k):
        big.sample_actions(out, s)
        traj.append(big.env_step(out)[0].clone())
    for i in (0, 63, 64, 129):
        one = _engine(1, lane_offset=i)
        one.env_reset()
        o1 = torch.empty(1, 7, dtype=torch.float32, device=DEV)
        for s in range(k):
            one.sample_actions(o1, s)
            o = one.env_step(o1)[0]
            assert torch.equal(o[0], traj[s][i]), (i, s)


def test_sample_actions_in_bounds():
    from pyflyt_amd.gym_envs import RocketLandingVecEnv

    env = RocketLandingVecEnv(4096, seed=4)
    lo = torch.tensor(LOW, device=DEV)
    seen_lo = torch.full((7,), 9.0, device=DEV)
    seen_hi = torch.full((7,), -9.0, device=DEV)
    for s in range(4):
        a = env.sample_actions(s)
        assert a.shape == (4096, 7)
        assert bool((a >= lo).all()) and bool((a <= 1.0).all())
        seen_lo = torch.minimum(seen_lo, a.min(0).values)
        seen_hi = torch.maximum(seen_hi, a.max(0).values)
    assert float((seen_lo - lo).abs().max()) < 1e-3 and float((seen_hi - 1.0).abs().max()) < 1e-3
    assert env.single_action_space.shape == (7,)
    env.close()


def test_facade_step_and_rollout():
    from pyflyt_amd.gym_envs import RocketLandingVecEnv

    env = RocketLandingVecEnv(256, seed=5, angle_representation="euler")
    obs, info = env.reset()
    assert obs.shape == (256, 29) and set(info.keys()) == {"out_of_bounds", "fatal_collision", "env_complete", "nonfinite"}
    assert float(obs[:, 11].min()) > 300.0  # a randomized drop from 0.8-0.9 x 500 m (z: index 11 in the euler layout)
    obs, r, te, tr, info = env.step(env.sample_actions(0))
    assert obs.shape == (256, 29) and r.shape == (256,)
    o, r, te, tr, a = env.engine.rollout(8)
    assert o.shape == (8, 256, 29) and a.shape == (8, 256, 7)
    env.close()

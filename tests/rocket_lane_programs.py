"""Lane programs for the mixed-wave Rocket-Landing replay (tests/test_gpu_rocket_landing.py, tests/test_cpu_rocket_landing.py).

A lane replays ONE recorded fixture (tests/golden/env_rocket_landing_*.npz) as a program of ops, one op per global call:
  IDLE        the lane's start delay: stepped with a zero action and zero draws, then reset from the host with zero draws; not compared
  RESET(ri)   reset from the host (a masked env_reset after the call's step launch) with the recording's reset ri; in the step launch
              of that call the lane is done (mode "off": it ended on the previous call) or fed zeros (the program's first op)
  STEP(k)     the recording's step k. Mode "same_step": a terminal step carries the inputs of the reset that follows it (`ri`), and
              the kernel resets the lane inside that call; mode "off": the reset is the next call's RESET op.
The program loops back to RESET(0) at the fixture's end; lane i starts `delay[i]` calls late, so lanes of one fixture are out of
phase and the 64 lanes of a wave do different things in the same launch. Everything here is a pure function of the fixtures:
numpy only, no device.
"""
from __future__ import annotations

import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IDLE, RESET, STEP = 0, 1, 2
Z_CONTACT = 2.7  # the replay's rule (test_gpu_rocket_landing.py): base z below it = the legs within reach of the pad or the floor
MIXED_FIXTURES = ("offpad", "land", "hard", "rest_tilt", "ceiling")  # one context: ceiling 20, quaternion, dense, options {}
N_LANES = 70
ZI = 12  # base z in the quaternion layout


def load(name):
    """the fixture as a dict of arrays (an NpzFile decompresses a member on every access)"""
    with np.load(os.path.join(GOLD, f"env_rocket_landing_{name}.npz")) as g:
        return {k: g[k] for k in g.files}


def lane_delays(n=N_LANES, n_fix=len(MIXED_FIXTURES)):
    """Lane i runs fixture i % n_fix; its j-th lane (j = i // n_fix) starts 5 j + (i % n_fix) calls late -- 0 to 69 over 70 lanes.
    test_cpu_rocket_landing.py::test_mixed_schedule_coverage proves what this choice has to deliver."""
    return np.array([5 * (i // n_fix) + (i % n_fix) for i in range(n)], dtype=np.int64)


def program(g, mode):
    """One pass of fixture g as a list of (kind, k, ri)."""
    assert mode in ("off", "same_step")
    K = len(g["action"])
    resets = [int(k) for k in g["reset_before"]]
    assert not (bool(g["term"][K - 1]) or bool(g["trunc"][K - 1]))  # (a pass ends on a live lane: the loop's RESET(0) is a host reset)
    prog, ri = [(RESET, -1, 0)], 1
    for k in range(K):
        if k in resets and mode == "off":
            prog.append((RESET, -1, ri))
            ri += 1
        if mode == "same_step" and (k + 1) in resets:
            prog.append((STEP, k, ri))
            ri += 1
        else:
            prog.append((STEP, k, -1))
    assert ri == len(g["reset_obs"])
    return prog


def schedule(fixtures, mode, n=N_LANES, delays=None, calls=None):
    """kind / k / ri / fix as [calls, n] integer arrays. calls=None: the largest delay plus the longest pass."""
    progs = [program(g, mode) for g in fixtures]
    delays = lane_delays(n, len(fixtures)) if delays is None else np.asarray(delays)
    if calls is None:
        calls = int(delays.max()) + max(len(p) for p in progs)
    S = dict(kind=np.zeros((calls, n), np.int8), k=np.full((calls, n), -1, np.int64), ri=np.full((calls, n), -1, np.int64),
             fix=np.array([i % len(fixtures) for i in range(n)]), delays=delays, period=np.array([len(p) for p in progs]), mode=mode)
    for i in range(n):
        p = progs[i % len(fixtures)]
        for t in range(int(delays[i]), calls):
            S["kind"][t, i], S["k"][t, i], S["ri"][t, i] = p[(t - int(delays[i])) % len(p)]
    return S


def is_contact_step(g, k, zi=ZI):
    """replay's rule for the steps held to RTOL_IMPACT"""
    return bool(g["info_col"][k]) or g["obs"][k][zi] < Z_CONTACT or (k > 0 and g["obs"][k - 1][zi] < Z_CONTACT)


def assemble(S, fixtures):
    """The per-call inputs and expectations of schedule S: float32 inputs laid out as the engine takes them, float64 references.
    u_targets is the same on every call: in inject mode begin_reset takes the six rows as the spawn pose itself."""
    T, n = S["kind"].shape
    D = fixtures[0]["obs"].shape[1]
    A = dict(actions=np.zeros((T, n, 7), np.float32), xi=np.zeros((T, 6, n), np.float32), xi_reset=np.zeros((T, 20, n), np.float32),
             u_targets=np.zeros((6, n), np.float32), reset_mask=np.zeros((T, n), bool),
             ref_obs=np.zeros((T, n, D)), ref_final=np.zeros((T, n, D)), ref_reward=np.zeros((T, n)), ref_term=np.zeros((T, n), bool),
             ref_trunc=np.zeros((T, n), bool), ref_info=np.zeros((T, n), np.int64), impact=np.zeros((T, n), bool))
    for i in range(n):
        g = fixtures[S["fix"][i]]
        A["u_targets"][:3, i], A["u_targets"][3:, i] = g["start_pos"], g["start_orn"]
        assert not np.asarray(g["reset_u"]).any() and int(g["options"]) == 0  # (recorded with options {}: the pose is start_pos / start_orn)
        for t in range(T):
            kind, k, ri = int(S["kind"][t, i]), int(S["k"][t, i]), int(S["ri"][t, i])
            A["reset_mask"][t, i] = kind != STEP
            if ri >= 0:
                A["xi_reset"][t, :, i] = g["reset_xi"][ri]
            if kind == RESET:
                A["ref_obs"][t, i] = g["reset_obs"][ri]
            if kind == STEP:
                A["actions"][t, i] = g["action"][k]
                A["xi"][t, :, i] = np.nan_to_num(g["xi"][k])
                A["ref_reward"][t, i], A["ref_term"][t, i], A["ref_trunc"][t, i] = g["reward"][k], g["term"][k], g["trunc"][k]
                A["ref_info"][t, i] = 8 * int(g["info_col"][k]) + 16 * int(g["info_oob"][k]) + 32 * int(g["info_complete"][k])  # _lib.F_INFO_*
                A["impact"][t, i] = is_contact_step(g, k)
                if ri >= 0:  # same_step: the terminal observation in final_obs, the reset's in obs
                    A["ref_final"][t, i], A["ref_obs"][t, i] = g["obs"][k], g["reset_obs"][ri]
                else:
                    A["ref_obs"][t, i] = g["obs"][k]
    return A


def categories(S, fixtures, names):
    """Which lanes are, on each call, in each of the five situations the mixed replay is for: [calls, n] bool arrays."""
    T, n = S["kind"].shape
    C = {c: np.zeros((T, n), bool) for c in ("floor", "pad", "flight", "reset", "done_or_idle")}
    for i in range(n):
        g, name = fixtures[S["fix"][i]], names[S["fix"][i]]
        for t in range(T):
            kind, k, ri = int(S["kind"][t, i]), int(S["k"][t, i]), int(S["ri"][t, i])
            if kind == STEP:
                z = g["obs"][k][ZI]
                C["floor"][t, i] = name == "offpad" and bool(g["info_col"][k])
                C["pad"][t, i] = g["obs"][k][-1] == 1.0 or (name in ("land", "hard") and z < Z_CONTACT)
                C["flight"][t, i] = not is_contact_step(g, k)
                C["reset"][t, i] = ri >= 0  # reset by the kernel inside this call
            elif kind == RESET:
                # the host's masked reset launch; in the call's step launch the lane sits out as a done lane (mode "off", ri > 0).
                # Mode "same_step" counts only the resets the kernel does inside a step call.
                C["reset"][t, i] = S["mode"] == "off"
                C["done_or_idle"][t, i] = S["mode"] == "off" and ri > 0
            else:
                C["done_or_idle"][t, i] = True
    return C


def distinct_witnesses(sets):
    """Can each of the sets name a lane of its own? (five small sets: depth-first)"""
    def rec(j, used):
        if j == len(sets):
            return True
        return any(rec(j + 1, used | {x}) for x in sets[j] if x not in used)
    return rec(0, frozenset())

"""Rocket-Landing without a GPU: the parameter block, the spaces, agent_hz validation, the fp64 landing-pad model
(tests/golden/pad_bullet.py) the fixtures are recorded on, what each fixture is for, and the schedule of the mixed-wave replay
(tests/rocket_lane_programs.py)."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from pyflyt_amd import _lib as L  # noqa: E402
from pyflyt_amd.params import build_params  # noqa: E402

GOLD = os.path.join(HERE, "golden")
FIXTURES = ("random", "euler", "offpad", "land", "hard", "timeout", "ceiling", "lateral", "rest_tilt")


def test_params_fields():
    P = build_params("rocket", "rocket_landing")
    assert P.task == L.TASK_ROCKET_LANDING == 5 and P.vehicle == L.ROCKET and P.flight_mode == 0
    assert P.env_step_ratio == 3 and P.max_steps == 1200 and P.settle_steps == 10 and P.ticks_per_control == 2
    assert list(P.pad_pos) == pytest.approx([0.0, 0.0, 0.1]) and P.pad_radius == 2.0 and P.pad_half_height == pytest.approx(0.05)
    assert P.pad_pos[2] + P.pad_half_height == pytest.approx(0.15)  # the pad's top face
    assert P.ceiling == 500.0 and P.max_displacement == 200.0
    assert P.rl_reset_options == L.RL_RANDOMIZE_DROP | L.RL_ACCELERATE_DROP == 3
    assert list(P.start_pos) == pytest.approx([0.0, 0.0, 450.0])  # rocket_landing_env.py:56
    assert P.rocket.starting_fuel_ratio == pytest.approx(0.05)
    P = build_params("rocket", "rocket_landing", ceiling=20.0, max_displacement=5.0, agent_hz=60, max_duration_seconds=2.0, reset_options=0,
                     world_options=dict(landing_pad_pos=(1.0, 2.0, 0.3), landing_pad_radius=1.5, landing_pad_length=0.2))
    assert P.env_step_ratio == 2 and P.max_steps == 120 and P.ceiling == 20.0 and P.max_displacement == 5.0 and P.rl_reset_options == 0
    assert list(P.pad_pos) == pytest.approx([1.0, 2.0, 0.3]) and P.pad_radius == 1.5 and P.pad_half_height == pytest.approx(0.1)


def test_abi_size_and_version():
    assert L.PF_ABI_VERSION == 10
    so = L.lib() if os.path.exists(L.LIB_PATH) else None
    if so is not None:
        assert so.pf_sizeof_params() == C.sizeof(L.PfParams)
        assert so.pf_abi_version() == 10
    assert L.PfParams.pad_pos.offset > L.PfParams.rocket.offset  # the new fields at the end of the block
    assert L.PfParams.rl_reset_options.offset + 4 <= C.sizeof(L.PfParams)


def test_other_rocket_tasks_refused():
    for task in ("hover", "waypoints", "ma_hover", "dogfight"):
        with pytest.raises(ValueError):
            build_params("rocket", task)
    with pytest.raises(ValueError):
        build_params("quadx", "rocket_landing")
    with pytest.raises(ValueError):
        build_params("rocket", "rocket_landing", flight_mode=1)
    with pytest.raises(ValueError):
        build_params("rocket", "rocket_landing", reset_options=4)


@pytest.mark.parametrize("hz,msg", [(50, "try 40 or 60"), (70, "try 60 or 120")])
def test_agent_hz_validation(hz, msg):
    with pytest.raises(ValueError, match=f"`agent_hz` must be round denominator of 120, {msg}."):
        build_params("rocket", "rocket_landing", agent_hz=hz)


def test_spaces_and_obs_width():
    from pyflyt_amd.gym_envs import RocketLandingVecEnv
    from pyflyt_amd.gym_envs.vector_envs import _REGISTRY

    assert RocketLandingVecEnv not in _REGISTRY.values()  # (make_vec: a follow-up, see the class docstring)
    env = RocketLandingVecEnv.__new__(RocketLandingVecEnv)  # the spaces without a device context
    env.num_envs = 3

    class _Eng:
        params = build_params("rocket", "rocket_landing")

    env.engine = _Eng()
    env._make_obs_space()
    assert env.single_observation_space.shape == (30,)
    assert env.single_observation_space.low[-1] == 0.0 and env.single_observation_space.high[-1] == 1.0
    _Eng.params = build_params("rocket", "rocket_landing", angle_representation="euler")
    env._make_obs_space()
    assert env.single_observation_space.shape == (29,) and env.observation_space.shape == (3, 29)
    assert RocketLandingVecEnv._LOW == (-1.0, -1.0, -1.0, 0.0, 0.0, -1.0, -1.0)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_shapes(name):
    g = np.load(os.path.join(GOLD, f"env_rocket_landing_{name}.npz"))
    k = len(g["action"])
    D = 29 if int(g["angle_repr"]) == 0 else 30
    assert g["action"].shape == (k, 7) and g["obs"].shape == (k, D) and g["xi"].shape == (k, 6)
    assert g["reset_u"].shape[1] == 6 and g["reset_xi"].shape[1] == 20 and len(g["reset_obs"]) == len(g["reset_before"]) + 1
    assert set(np.unique(g["obs"][:, -1])) <= {0.0, 1.0}


def test_fixture_outcomes():
    """what each fixture is for (gen_rocket_landing.py)"""
    f = {n: np.load(os.path.join(GOLD, f"env_rocket_landing_{n}.npz")) for n in FIXTURES}
    assert f["random"]["info_col"].any() and int(f["random"]["options"]) == -1
    assert f["euler"]["obs"].shape[1] == 29 and bool(f["euler"]["sparse"])
    land = f["land"]
    k = int(np.argmax(land["info_complete"]))
    assert land["info_complete"][k] and land["trunc"][k] and not land["info_col"][: k + 1].any()
    assert land["reward"][k] > 7.0  # the pad bonus and the completion bonus
    hard = f["hard"]
    k = int(np.argmax(hard["info_col"]))
    assert hard["term"][k] and hard["obs"][k][12] > 2.5  # on the pad (not the floor, not below z = 0): the pad branch's verdict
    off = f["offpad"]
    k = int(np.argmax(off["info_col"]))
    assert off["term"][k] and off["obs"][k][12] < 2.5 and not off["obs"][:, -1].any()
    ends = lambda g, key: np.nonzero(g[key])[0].tolist()  # noqa: E731
    nothing_else = lambda g, *keys: not any(g[k].any() for k in ("term", "trunc", "info_oob", "info_col", "info_complete") if k not in keys)  # noqa: E731
    # the time limit, in free flight: a 0.5 s episode is max_steps = 20, and `step_count > max_steps` lets 22 steps through
    t = f["timeout"]
    assert float(t["max_duration_seconds"]) == 0.5 and int(t["options"]) == -1
    assert ends(t, "trunc") == [21, 43] and t["reset_before"].tolist() == [22, 44] and nothing_else(t, "trunc")
    assert t["obs"][:, 12].min() > 300.0 and not t["obs"][:, -1].any()
    # the ceiling branch of out_of_bounds: z crosses 20 m with the rocket over the pad
    c = f["ceiling"]
    assert ends(c, "term") == ends(c, "info_oob") == [16, 33, 50] and nothing_else(c, "term", "info_oob")
    assert all(c["obs"][k][12] > float(c["ceiling"]) == 20.0 > c["obs"][k - 1][12] for k in (16, 33, 50))
    assert np.linalg.norm(c["obs"][:, 10:12], axis=1).max() < float(c["max_displacement"])
    # the lateral branch: 3 m from the axis, far below the ceiling
    la = f["lateral"]
    assert ends(la, "term") == ends(la, "info_oob") == [61] and nothing_else(la, "term", "info_oob")
    assert float(la["max_displacement"]) == 3.0 and np.linalg.norm(la["obs"][61][10:12]) > 3.0 > np.linalg.norm(la["obs"][60][10:12])
    assert la["obs"][:, 12].max() < float(la["ceiling"]) == 60.0
    # a pad contact that lasts: the pad bit on EVERY step, the pad bonus on every step, env_complete once the rocket is at rest
    r = f["rest_tilt"]
    assert int(r["obs"][:, -1].sum()) == len(r["action"]) == 80
    assert ends(r, "trunc") == ends(r, "info_complete") == [18, 37, 56, 75] and nothing_else(r, "trunc", "info_complete")
    assert r["reward"].min() > 4.0 and all(r["reward"][k] > r["reward"][k - 1] + 2.9 for k in (18, 37, 56, 75))  # +5 each step, +3 on completion
    assert np.abs(r["start_orn"] - np.array([0.01, -0.01, 0.5])).max() == 0.0


# ------------------------------------------------------------------ the mixed-wave replay's schedule (tests/rocket_lane_programs.py)
@pytest.mark.parametrize("mode", ["off", "same_step"])
def test_mixed_schedule_coverage(mode):
    """The schedule is a pure function of the fixtures: every (fixture, step) and every recorded reset is visited, every lane
    completes a pass, and there are calls on which the first wave (lanes 0..63) holds, in five different lanes at once, a lane on a
    floor-collision step, one on a pad-contact step, one in free flight, one being reset and one that is done or idle."""
    import rocket_lane_programs as RLP

    names = RLP.MIXED_FIXTURES
    fixtures = [RLP.load(n) for n in names]
    S = RLP.schedule(fixtures, mode)
    T, n = S["kind"].shape
    assert n == RLP.N_LANES == 70 and T == int(S["delays"].max()) + int(S["period"].max()) and T < 380
    assert len(set(S["delays"].tolist())) == n  # no two lanes in phase
    for fi, g in enumerate(fixtures):
        lanes = S["fix"] == fi
        steps = S["k"][:, lanes][S["kind"][:, lanes] == RLP.STEP]
        assert set(steps.tolist()) == set(range(len(g["action"]))), names[fi]
        assert set(S["ri"][:, lanes][S["ri"][:, lanes] >= 0].tolist()) == set(range(len(g["reset_obs"]))), names[fi]
    for i in range(n):  # a full pass: the program's first op to its last, in order
        d, L = int(S["delays"][i]), int(S["period"][S["fix"][i]])
        assert d + L <= T and (S["kind"][:d, i] == RLP.IDLE).all() and (S["kind"][d:, i] != RLP.IDLE).all()
        assert S["kind"][d, i] == RLP.RESET and S["ri"][d, i] == 0
        ks = S["k"][d:d + L, i][S["kind"][d:d + L, i] == RLP.STEP]
        assert ks.tolist() == list(range(len(fixtures[S["fix"][i]]["action"])))
    C = RLP.categories(S, fixtures, names)
    order = ("floor", "pad", "flight", "reset", "done_or_idle")
    full = [t for t in range(T) if RLP.distinct_witnesses([set(np.nonzero(C[c][t, :64])[0].tolist()) for c in order])]
    print(f"mode {mode}: {T} calls, {len(full)} of them with all five situations in five lanes of the first wave (first {full[:5]})")
    assert len(full) >= 3, full
    # and the situations the five-way calls do not need: a lane resets inside a call while wave-mates step on (same_step), every
    # fixture meets every other one's contact steps out of phase
    if mode == "same_step":
        assert ((C["reset"] & (S["kind"] == RLP.STEP))[:, :64].any(1) & C["flight"][:, :64].any(1)).sum() > 50
    A = RLP.assemble(S, fixtures)
    assert A["reset_mask"][S["kind"] != RLP.STEP].all() and not A["reset_mask"][S["kind"] == RLP.STEP].any()
    assert np.isfinite(A["xi"]).all() and A["impact"].any() and (~A["impact"][S["kind"] == RLP.STEP]).any()


# ------------------------------------------------------------------ the fp64 pad model (tests/golden/pad_bullet.py)
@pytest.fixture(scope="module")
def pad_client():
    import pad_bullet

    return pad_bullet


def _rocket_body(pad_bullet, pos):
    """A Rocket-shaped free body (the collision cylinders, fin boxes and yawed legs of rocket.urdf, params.ROCKET) next to the
    ground slab and the landing pad, in the fp64 client; engine off."""
    from oracle import fake_bullet
    from pyflyt_amd.params import ROCKET, WORLD

    cl = pad_bullet.PadBulletClient()
    cl.setGravity(0.0, 0.0, -9.81)
    cl.loadURDF("plane.urdf", useFixedBase=True)
    link = fake_bullet._Link("pad")
    link.cyls.append((np.zeros(3), WORLD["landing_pad_radius"], 0.5 * WORLD["landing_pad_length"]))
    pid = cl._next_id
    cl._bodies[pid] = fake_bullet._Body([link], True, WORLD["landing_pad_pos"], (0.0, 0.0, 0.0, 1.0))
    cl._next_id += 1
    cl._pads.append(pid)
    base = fake_bullet._Link("base")
    base.mass = sum(l[0] for l in ROCKET["links"]) - ROCKET["links"][1][0] * (1.0 - 0.05)
    base.inertia = np.diag([400.0, 400.0, 2.0])
    for c, r, length in ROCKET["collision_cylinders"]:
        base.cyls.append((np.array(c), r, 0.5 * length))
    for c, size in ROCKET["collision_boxes"]:
        base.boxes.append((np.array(c), 0.5 * np.array(size)))
    legs = []
    for c, size, yaw in ROCKET["collision_boxes_yawed"]:  # (a massless link per leg, yawed about the base z axis)
        leg = fake_bullet._Link("leg")
        cy, sy = np.cos(yaw), np.sin(yaw)
        leg.rot = np.array([[cy, -sy, 0.0], [sy, cy, 0.0], [0.0, 0.0, 1.0]])
        leg.joint_origin = np.array(c, dtype=np.float64)
        leg.boxes.append((np.zeros(3), 0.5 * np.array(size)))
        legs.append(leg)
    rid = cl._next_id
    cl._bodies[rid] = fake_bullet._Body([base] + legs, False, pos, (0.0, 0.0, 0.0, 1.0))
    cl._next_id += 1
    return cl, pid, rid


def _settle(cl, n):
    for _ in range(n):
        cl.stepSimulation()


def test_pad_model_rests_on_the_pad(pad_client):
    """set down on the pad, the rocket comes to rest with its legs on the top face (z = 0.15): base z = 0.15 + 2.425 - slop"""
    cl, pid, rid = _rocket_body(pad_client, (0.1, -0.2, 2.60))
    _settle(cl, 480)
    b = cl._bodies[rid]
    assert b.p[2] == pytest.approx(2.575 - cl.contact_slop, abs=2e-4), b.p
    assert np.linalg.norm(b.v) < 2e-3 and np.linalg.norm(b.w) < 2e-3
    pairs = {(c[1], c[2]) for c in cl.getContactPoints()}
    assert (pid, rid) in pairs and (0, rid) not in pairs  # the pad, not the floor


def test_pad_model_beside_the_pad(pad_client):
    """beside the pad the legs reach the floor: a floor contact, no pad contact, resting at z = 2.425 - slop"""
    cl, pid, rid = _rocket_body(pad_client, (4.0, 1.0, 2.45))
    _settle(cl, 480)
    b = cl._bodies[rid]
    assert b.p[2] == pytest.approx(2.425 - cl.contact_slop, abs=2e-4), b.p
    pairs = {(c[1], c[2]) for c in cl.getContactPoints()}
    assert (0, rid) in pairs and (pid, rid) not in pairs

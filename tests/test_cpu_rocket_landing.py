"""Rocket-Landing without a GPU: the parameter block, the spaces, agent_hz validation, and the fp64 landing-pad model
(tests/golden/pad_bullet.py) the fixtures are recorded on."""
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
FIXTURES = ("random", "euler", "offpad", "land", "hard")


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

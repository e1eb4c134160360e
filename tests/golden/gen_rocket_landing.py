"""gen_rocket_landing.py -- the Rocket-Landing fixtures tests/golden/env_rocket_landing_*.npz.

RUN ONLY IN THE BUILD CONTAINER (needs the reference):  python tests/golden/gen_rocket_landing.py [--out DIR] [name ...]

Installs ref_stubs' module stand-ins, swaps in pad_bullet.PadBulletClient (fake_bullet with the landing pad) and runs the
reference's own RocketLandingEnv (gym_envs/rocket_envs/rocket_landing_env.py). Per step it records the action, observation,
reward, terminated, truncated, the three info keys and the raw booster-noise draws (NaN padded to the step's 6 ticks); per reset
the six spawn uniforms as the reference takes them (x, y, z, roll, pitch, yaw -- zeros without randomize_drop), the settle draws
and the reset observation. Every input is float32-exact (ref_stubs.RecordingRNG.F32): the device takes float32 actions and draws.
The .npz files hold data only.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_stubs  # noqa: E402

ref_stubs.install()
import pad_bullet  # noqa: E402

sys.modules["pybullet_utils.bullet_client"].BulletClient = pad_bullet.PadBulletClient  # (before the Aviary class is defined)
from PyFlyt.gym_envs.rocket_envs.rocket_landing_env import RocketLandingEnv  # noqa: E402

OUT_DIR = HERE
TICKS = 6  # env_step_ratio 3 x 2 physics ticks per Aviary step at agent_hz 40


def save(name, **arrays):
    path = os.path.join(OUT_DIR, name + ".npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in arrays.items()})
    print(f"wrote {path}: " + ", ".join(f"{k}{np.asarray(v).shape}" for k, v in arrays.items()))


def run(name, n_steps, seed, policy, options="default", env_kwargs=None, setup=None):
    """options: "default" = reset(options=None) (what gymnasium.make passes: randomize_drop and accelerate_drop), or a dict.
    setup(env): called after each reset (a start pose by hand goes through env.start_pos / start_orn before the reset instead)."""
    ref_stubs.RecordingRNG.F32 = True
    try:
        kw = dict(env_kwargs or {})
        env = RocketLandingEnv(**kw)
        opts = None if options == "default" else dict(options)
        rec = dict(action=[], obs=[], reward=[], term=[], trunc=[], xi=[], info_oob=[], info_col=[], info_complete=[],
                   reset_before=[], reset_obs=[], reset_u=[], reset_xi=[])

        def do_reset(s):
            if setup is not None:
                setup(env)
            obs, _ = env.reset(seed=s, options=opts)
            r = env.np_random
            u = r.drain("uniform")
            rec["reset_u"].append(u if len(u) else np.zeros(6))
            rec["reset_xi"].append(r.drain("normal"))
            rec["reset_obs"].append(np.array(obs, dtype=np.float64))

        do_reset(seed)
        rng = np.random.default_rng(seed + 77)
        ep_seed, need = seed, False
        for k in range(n_steps):
            if need:
                ep_seed += 1
                rec["reset_before"].append(k)
                do_reset(ep_seed)
            a = np.asarray(policy(env, rng, k), dtype=np.float64).astype(np.float32).astype(np.float64)
            obs, r, te, tr, info = env.step(a)
            x = env.np_random.drain("normal")
            rec["action"].append(a)
            rec["obs"].append(np.array(obs, dtype=np.float64))
            rec["reward"].append(r)
            rec["term"].append(te)
            rec["trunc"].append(tr)
            rec["xi"].append(np.concatenate([x, np.full(TICKS - len(x), np.nan)]))
            rec["info_oob"].append(info["out_of_bounds"])
            rec["info_col"].append(info["fatal_collision"])
            rec["info_complete"].append(info["env_complete"])
            need = bool(te or tr)
        out = {k: np.array(v) for k, v in rec.items()}
        out.update(seed=seed, options=np.array(-1 if options == "default" else
                                               (1 if opts.get("randomize_drop") else 0) | (2 if opts.get("accelerate_drop") else 0)),
                   ceiling=np.array(env.ceiling), max_displacement=np.array(env.max_displacement),
                   angle_repr=np.array(env.angle_representation), sparse=np.array(env.sparse_reward),
                   start_pos=np.array(env.start_pos, dtype=np.float64).reshape(-1), start_orn=np.array(env.start_orn, dtype=np.float64).reshape(-1))
        if "max_duration_seconds" in kw:  # (the env keeps max_steps only; the default, 60 s, is not stored)
            out.update(max_duration_seconds=np.array(float(kw["max_duration_seconds"])))
        return out
    finally:
        ref_stubs.RecordingRNG.F32 = False


def uniform_action(env, rng, k):
    return rng.uniform(env.action_space.low, env.action_space.high)


def idle_action(env, rng, k):  # engine off, fins neutral: a free fall
    return np.zeros(7)


def pulsed_descent(v_target, z_cut):
    """A scripted descent. The booster's least thrust (min_thrust, rocket.yaml) lifts the rocket with 5 % of its fuel, so it cannot
    hover: the ignition pulses (throttle 0) whenever the vertical speed is below the target for the height, and stays off from
    z_cut down (the legs about to touch the pad)."""
    def f(env, rng, k):
        vz = float(env.ground_lin_vel[2])
        z = float(env.lin_pos[2])
        ign = 1.0 if (z > z_cut and vz < v_target(z)) else 0.0
        return np.array([0.0, 0.0, 0.0, ign, 0.0, 0.0, 0.0])
    return f


def constant_action(a):
    def f(env, rng, k):
        return np.array(a, dtype=np.float64)
    return f


def start_at(pos, orn=(0.0, 0.0, 0.0)):
    def f(env):
        env.start_pos = np.array([pos], dtype=np.float64)
        env.start_orn = np.array([orn], dtype=np.float64)
    return f


GROUPS = {}


def group(fn):
    GROUPS[fn.__name__[4:]] = fn
    return fn


@group
def gen_random():
    # default options (randomized drop at -100 m/s from 0.8-0.9 x 500 m), random actions: ends in a fatal collision
    save("env_rocket_landing_random", **run("random", 600, 11, uniform_action))


@group
def gen_euler():
    save("env_rocket_landing_euler", **run("euler", 300, 12, uniform_action,
                                          env_kwargs=dict(angle_representation="euler", sparse_reward=True)))


@group
def gen_offpad():
    # dropped beside the pad: the legs meet the floor -> fatal_collision from the base env
    save("env_rocket_landing_offpad", **run("offpad", 40, 13, idle_action, options={}, env_kwargs=dict(ceiling=20.0),
                                           setup=start_at((4.0, 1.0, 3.0))))


@group
def gen_land():
    # a small ceiling, options={}: a throttle controller brings the rocket down onto the pad below 1 m/s and holds it -> env_complete
    def v_target(z):
        return -max(0.4, min(4.0, 0.8 * (z - 2.575)))
    save("env_rocket_landing_land", **run("land", 300, 14, pulsed_descent(v_target, 2.62), options={}, env_kwargs=dict(ceiling=20.0),
                                         setup=start_at((0.3, -0.2, 8.0))))


@group
def gen_hard():
    # onto the pad too fast: fatal_collision from the pad branch (previous speed > 1 m/s)
    save("env_rocket_landing_hard", **run("hard", 60, 15, idle_action, options={}, env_kwargs=dict(ceiling=20.0),
                                         setup=start_at((0.2, 0.1, 4.0))))


@group
def gen_timeout():
    # a half-second episode (20 steps at 40 Hz), default options, random actions: truncated by the time limit in free flight, twice
    save("env_rocket_landing_timeout", **run("timeout", 50, 21, uniform_action, env_kwargs=dict(max_duration_seconds=0.5)))


@group
def gen_ceiling():
    # full throttle from 17 m under a 20 m ceiling: out_of_bounds through the ceiling branch, three times
    save("env_rocket_landing_ceiling", **run("ceiling", 60, 22, constant_action((0, 0, 0, 1, 1, 0, 0)), options={}, env_kwargs=dict(ceiling=20.0),
                                            setup=start_at((0.5, 0.5, 17.0))))


@group
def gen_lateral():
    # the gimbal hard over at 30 % throttle, 2 m from the axis with 3 m allowed: out_of_bounds through the lateral branch
    save("env_rocket_landing_lateral", **run("lateral", 120, 23, constant_action((0, 0, 0, 1, 0.3, 1, 0)), options={},
                                            env_kwargs=dict(ceiling=60.0, max_displacement=3.0), setup=start_at((2.0, 0.0, 30.0))))


@group
def gen_rest_tilt():
    # set down on the pad a hair's breadth up, slightly tilted and yawed, engine off: a pad contact that lasts the whole episode (the
    # pad bit and the +5 - 0.3 |gvz| bonus on every step) until the rocket has come to rest -> env_complete, four times
    save("env_rocket_landing_rest_tilt", **run("rest_tilt", 80, 26, idle_action, options={}, env_kwargs=dict(ceiling=20.0),
                                              setup=start_at((0.3, -0.4, 2.60), (0.01, -0.01, 0.5))))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--out":
        OUT_DIR = sys.argv[2]
        del sys.argv[1:3]
    for name in (sys.argv[1:] or list(GROUPS)):
        GROUPS[name]()

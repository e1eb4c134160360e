"""The stepwise closed loop at small sizes, where the host was expected to be the bound: at 65 536 lanes the loop's Python hides behind
the kernels (tools/bench_policy_act.py leg S, tools/bench_ma_collect.py leg W). Measured, it hides here too -- a Fixedwing step is
31 us at one wave per SIMD, a dogfight step 318 us, the Python 2 us and 4 us (closed_loop_stub_cost.py times that alone, on a CPU) --
so this is the loop end to end at the smallest sizes anyone trains at, not its host cost.

    steps   BatchEngine.rollout_policy_steps(policy, 100) on Fixedwing-Waypoints, n = 1024:  100 x (pf_policy_act, pf_env_step)
    worlds  MAFixedwingDogfightEnv(team_size=2, num_envs=256).rollout(policy, 64):            64 x (pf_policy_act, pf_env_step,
                                                                                              pf_world_sync, pf_env_reset)

Wall-clock microseconds per env step: one untimed call, then samples of at least 0.5 s of calls between two torch.cuda.synchronize(),
the median of `--repeats` samples per leg (default 3). Prints one JSON line. For an A/B of two trees' Python on one library, run it
from each tree with PF_LIB_PATH naming the library (profiles/closed_loop/nothing_moved.txt)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import pyflyt_amd  # noqa: E402
from pyflyt_amd import MLPPolicy, build_params  # noqa: E402
from pyflyt_amd.engine import BatchEngine  # noqa: E402
from pyflyt_amd.pz_envs import MAFixedwingDogfightEnv  # noqa: E402

DEV = "cuda:0"


def policy(eng):
    torch.manual_seed(0)
    nn = torch.nn
    net = nn.Sequential(nn.Linear(eng.obs_dim, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, eng.action_dim)).to(DEV)
    return MLPPolicy.from_torch(net, log_std=torch.full((eng.action_dim,), -1.0, device=DEV))


def steps_leg():
    k = 100
    eng = BatchEngine(build_params("fixedwing", "waypoints", seed=1), 1024, device=DEV)
    eng.env_reset()
    pol, step = policy(eng), [0]

    def call():
        eng.rollout_policy_steps(pol, k, step_index0=step[0])
        step[0] += k

    return call, k, eng


def worlds_leg():
    k = 64
    env = MAFixedwingDogfightEnv(team_size=2, num_envs=256, seed=1, max_duration_seconds=2.0, device=DEV)
    env.reset(seed=1)
    pol = policy(env.engine)
    return (lambda: env.rollout(pol, k)), k, env


def sample(call, k, min_seconds=0.5):
    """us per env step over at least `min_seconds` of calls."""
    torch.cuda.synchronize()
    calls, t0 = 0, time.perf_counter()
    while True:
        call()
        calls += 1
        if time.perf_counter() - t0 >= min_seconds:
            break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / (calls * k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    res = {"unit": "wall-clock us per env step", "python": os.path.dirname(pyflyt_amd.__file__)}
    for name, make in (("steps", steps_leg), ("worlds", worlds_leg)):
        call, k, owner = make()
        call()
        v = [sample(call, k) for _ in range(args.repeats)]
        owner.close()
        res[name] = {"us": sorted(v)[len(v) // 2], "min": min(v), "max": max(v), "samples": v}
    print(json.dumps(res))


if __name__ == "__main__":
    main()

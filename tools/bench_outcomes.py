"""What pf_episode_outcomes costs: microseconds per env step of the closed loops with outcomes=True against the same loops without, and the
trajectory-form call on its own.

    a  the world loop          MAFixedwingDogfightEnv 2 v 2, 16 384 copies (65 536 aircraft), env.rollout(policy, 64): outcomes off / on
    b  the stepwise loop       FixedwingWaypointsVecEnv, 65 536 lanes, NEXT_STEP, env.rollout(policy, 100): outcomes off / on
    c  the trajectory form     one BatchEngine.episode_outcomes call on the final_info rows of a 100-step SAME_STEP QuadX-Hover
                               trajectory of 65 536 lanes (us per call, and per step of the trajectory)

"Off" is the loop as it was before the feature: the same library (every existing kernel is identical in assembly,
profiles/outcomes/nothing_moved.txt) and the same Python but for one `is not None` test per step. The legs of a pair run on envs of
their own with the same arguments, in one process, on device events, each warmed up and timed over at least 0.5 s, alternated and
repeated (default five times): medians with the spread. No threshold: the numbers are recorded, not gated. Prints one JSON line and
writes profiles/outcomes/bench.json.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from pyflyt_amd import MLPPolicy  # noqa: E402
from pyflyt_amd.gym_envs.vector_envs import FixedwingWaypointsVecEnv, QuadXHoverVecEnv  # noqa: E402
from pyflyt_amd.pz_envs import MAFixedwingDogfightEnv  # noqa: E402

DEV = "cuda:0"


def policy_for(eng):
    torch.manual_seed(0)
    nn = torch.nn
    net = nn.Sequential(nn.Linear(eng.obs_dim, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, eng.action_dim)).to(DEV)
    return MLPPolicy.from_torch(net, log_std=torch.full((eng.action_dim,), -1.0, device=DEV))


def world_legs(copies, k=64):
    def make():
        env = MAFixedwingDogfightEnv(team_size=2, num_envs=copies, seed=1, max_duration_seconds=2.0, device=DEV)
        env.reset(seed=1)
        return env

    envs = [make(), make()]
    pol = policy_for(envs[0].engine)
    return {"off": lambda: envs[0].rollout(pol, k), "on": lambda: envs[1].rollout(pol, k, outcomes=True)}, envs, k


def stepwise_legs(lanes, k=100):
    def make():
        env = FixedwingWaypointsVecEnv(lanes, seed=1, autoreset_mode="next_step", device=DEV)
        env.reset(seed=1)
        return env

    envs = [make(), make()]
    pol = policy_for(envs[0].engine)
    return {"off": lambda: envs[0].rollout(pol, k), "on": lambda: envs[1].rollout(pol, k, outcomes=True)}, envs, k


def trajectory_leg(lanes, k=100):
    env = QuadXHoverVecEnv(lanes, seed=1, autoreset_mode="same_step", max_duration_seconds=2.0, device=DEV)
    env.reset(seed=1)
    eng = env.engine
    t = eng.collect_rollout(policy_for(eng), k)
    counts = torch.zeros(1, 16, dtype=torch.int64, device=DEV)
    out = torch.empty(k, lanes, dtype=torch.uint8, device=DEV)
    return {"call": lambda: eng.episode_outcomes(t["terminated"], t["truncated"], counts, info=t["final_info"], outcome_out=out)}, [env], 1


def time_leg(fn, per, min_seconds=0.5):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps, total = 0, 0.0
    while total < min_seconds * 1e3:
        a.record()
        fn()
        b.record()
        b.synchronize()
        total += a.elapsed_time(b)
        reps += 1
    return total * 1e3 / (reps * per)


def run(fns, envs, per, repeats):
    samples = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():  # (alternated)
            samples[name].append(time_leg(fn, per))
    for e in envs:
        e.close()
    return {name: {"us": sorted(v)[len(v) // 2], "min": min(v), "max": max(v), "samples": v} for name, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parts", default="a,b,c")
    args = ap.parse_args()
    parts = args.parts.split(",")
    res = {"lanes": args.lanes, "unit": "us per env step (c: us per call)"}
    if "a" in parts:
        res["a_world_loop"] = r = run(*world_legs(args.lanes // 4), args.repeats)
        r["added_us_per_step"] = r["on"]["us"] - r["off"]["us"]
    if "b" in parts:
        res["b_stepwise_fixedwing"] = r = run(*stepwise_legs(args.lanes), args.repeats)
        r["added_us_per_step"] = r["on"]["us"] - r["off"]["us"]
    if "c" in parts:
        res["c_trajectory_form_100_steps"] = r = run(*trajectory_leg(args.lanes), args.repeats)
        r["us_per_trajectory_step"] = r["call"]["us"] / 100
    line = json.dumps(res)
    print(line)
    if args.lanes == 65536 and parts == ["a", "b", "c"]:
        os.makedirs(os.path.join(ROOT, "profiles", "outcomes"), exist_ok=True)
        open(os.path.join(ROOT, "profiles", "outcomes", "bench.json"), "w").write(line + "\n")


if __name__ == "__main__":
    main()

"""What rollout() on the multi-agent envs buys: microseconds per env step of a closed policy loop on the team dogfight, 16 384 copies
of 2 v 2 (65 536 aircraft), 64-64 tanh policy with a Gaussian head, k = 64, 2 s episodes (60 steps: every window of 64 steps holds
truncations, deaths and resets of whole copies).

    W  env.rollout(policy, 64)          k x (pf_policy_act, pf_env_step, pf_world_sync, pf_env_reset), nothing waits for the host
    H  the loop a user writes today     64 x (engine.policy_act into the env's action views, env.step(dict) with its culling,
                                        env.done.all(dim=1) read on the host, env.reset_envs(...) when a copy has finished)

Both legs run on envs of their own with the same arguments, in one process, on device events, each warmed up and timed over at least
0.5 s, alternated and repeated (default five times). No threshold: the number is recorded, not gated. Prints one JSON line and writes
profiles/ma_collect/bench.json.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from pyflyt_amd import MLPPolicy  # noqa: E402
from pyflyt_amd.pz_envs import MAFixedwingDogfightEnv  # noqa: E402

K = 64
DEV = "cuda:0"


def make(num_envs):
    env = MAFixedwingDogfightEnv(team_size=2, num_envs=num_envs, seed=1, max_duration_seconds=2.0, device=DEV)
    env.reset(seed=1)
    return env


def legs(num_envs):
    envs = [make(num_envs), make(num_envs)]
    eng = envs[0].engine
    torch.manual_seed(0)
    nn = torch.nn
    net = nn.Sequential(nn.Linear(eng.obs_dim, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, eng.action_dim)).to(DEV)
    pol = MLPPolicy.from_torch(net, log_std=torch.full((eng.action_dim,), -1.0, device=DEV))
    E, A, W = envs[1].num_envs, envs[1].num_possible_agents, eng.action_dim
    act = torch.zeros(E * A, W, device=DEV)
    views = {ag: act.view(E, A, W)[:, i] for i, ag in enumerate(envs[1].possible_agents)}
    step = [0]

    def leg_w():
        envs[0].rollout(pol, K)

    def leg_h():
        env = envs[1]
        for _ in range(K):
            env.engine.policy_act(pol, step[0], out=act)
            step[0] += 1
            env.step(views)
            finished = env.done.all(dim=1)
            if bool(finished.any()):
                env.reset_envs(finished)

    return {"W": leg_w, "H": leg_h}, envs


def time_leg(fn, min_seconds=0.5):
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
    return total * 1e3 / (reps * K)  # us per env step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=16384)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    fns, envs = legs(args.num_envs)
    samples = {name: [] for name in fns}
    for _ in range(args.repeats):
        for name, fn in fns.items():
            samples[name].append(time_leg(fn))
    for e in envs:
        e.close()
    res = {"workload": f"team dogfight 2 v 2, {args.num_envs} copies ({4 * args.num_envs} aircraft), 64-64 tanh policy, Gaussian head, k = {K}, 60-step episodes",
           "unit": "us per env step", "legs": {"W": "env.rollout(policy, 64)", "H": "policy_act + env.step(dict) + reset_envs when a copy has finished"}}
    for name, v in samples.items():
        res[name] = {"us": sorted(v)[len(v) // 2], "min": min(v), "max": max(v), "samples": v}
    res["H_over_W"] = res["H"]["us"] / res["W"]["us"]
    line = json.dumps(res)
    print(line)
    if args.num_envs == 16384:
        os.makedirs(os.path.join(ROOT, "profiles", "ma_collect"), exist_ok=True)
        open(os.path.join(ROOT, "profiles", "ma_collect", "bench.json"), "w").write(line + "\n")


if __name__ == "__main__":
    main()

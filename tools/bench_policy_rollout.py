"""What pf_rollout_policy buys: microseconds per env step of a closed policy loop on QuadX-Hover, 64-64 tanh policy with a Gaussian head.

  A  engine.rollout_policy(policy, 100)                       the policy inside the rollout launch
  B  engine.rollout(100)                                      the env alone with sampled actions: the floor
  C  torch closed loop, eager: fp32 nn.Sequential + randn into a fixed action buffer, then env_step
  D  the loop of C, 100 steps captured in one HIP graph

One process, device events, every leg warmed up and timed over at least 0.5 s, the legs alternated and repeated three times. Prints
one JSON line and writes profiles/policy_rollout/bench.json. `--legs A` runs a subset (kernel times: run that under a kernel trace).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from pyflyt_amd import MLPPolicy, build_params  # noqa: E402
from pyflyt_amd.engine import BatchEngine  # noqa: E402

K = 100


def make_legs(n, legs):
    dev = "cuda:0"
    eng = BatchEngine(build_params("quadx", "hover", seed=1), n, device=dev)
    eng.env_reset()
    torch.manual_seed(0)
    nn = torch.nn
    net = nn.Sequential(nn.Linear(eng.obs_dim, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4)).to(dev)
    log_std = torch.full((4,), -1.0, device=dev)
    pol = MLPPolicy.from_torch(net, log_std=log_std)
    std = log_std.exp()
    act = torch.zeros(n, 4, device=dev)
    eps = torch.empty(n, 4, device=dev)
    step = [0]

    def leg_a():
        eng.rollout_policy(pol, K, step_index0=step[0])
        step[0] += K

    def leg_b():
        eng.rollout(K, step_index0=step[0], store_actions=True)
        step[0] += K

    def loop():
        with torch.no_grad():
            for _ in range(K):
                torch.addcmul(net(eng.obs), std, eps.normal_(), out=act)
                eng.env_step(act)

    out = {}
    if "A" in legs:
        out["A"] = leg_a
    if "B" in legs:
        out["B"] = leg_b
    if "C" in legs:
        out["C"] = loop
    if "D" in legs:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            loop()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            loop()
        out["D"] = g.replay
    return out, eng


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
    ap.add_argument("--legs", default="ABCD")
    ap.add_argument("--sizes", default="65536,524288")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    res = {"workload": "QuadX-Hover, 64-64 tanh policy, Gaussian head, k = 100", "unit": "us per env step", "sizes": {}}
    for n in (int(x) for x in args.sizes.split(",")):
        legs, eng = make_legs(n, args.legs)
        samples = {name: [] for name in legs}
        for _ in range(args.repeats):
            for name, fn in legs.items():
                samples[name].append(time_leg(fn))
        res["sizes"][str(n)] = {name: {"us_per_step": sorted(v)[len(v) // 2], "min": min(v), "max": max(v), "samples": v} for name, v in samples.items()}
        del legs
        eng.close()
    line = json.dumps(res)
    print(line)
    if set(args.legs) == set("ABCD"):
        os.makedirs(os.path.join(ROOT, "profiles", "policy_rollout"), exist_ok=True)
        open(os.path.join(ROOT, "profiles", "policy_rollout", "bench.json"), "w").write(line + "\n")


if __name__ == "__main__":
    main()

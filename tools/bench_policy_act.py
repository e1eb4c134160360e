"""What pf_policy_act buys: microseconds per env step of a closed policy loop where pf_rollout_policy has no launch, 64-64 tanh policy
with a Gaussian head, k = 100.

  Fixedwing-Waypoints
    S  engine.rollout_policy_steps(policy, 100)               k x (pf_policy_act, pf_env_step): the stepwise closed loop
    E  100 x env_step on a fixed action buffer                the env alone: the floor
    C  torch closed loop, eager: fp32 nn.Sequential + randn into a fixed action buffer, then env_step
    D  the loop of C, 100 steps captured in one HIP graph     (C and D: tools/bench_policy_rollout.py's legs, the best there was)
  QuadX-Hover
    F  engine.rollout_policy(policy, 100)                     the fused launch
    S  engine.rollout_policy_steps(policy, 100)               the stepwise loop on the same env
  The act launch alone
    us per pf_policy_act call at D = 21 (Hover) and D = 123 (an eight-aircraft dogfight, six-wide actions), 100 calls per sample,
    against FLOPs / 157.3 TF + 1.42 us (the matrix rate and the launch floor).

One process, device events, every leg warmed up and timed over at least 0.5 s, the legs alternated and repeated three times. Prints
one JSON line and writes profiles/policy_act/bench.json.
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
DEV = "cuda:0"
MATRIX_TF, LAUNCH_US = 157.3, 1.42


def nets(eng):
    torch.manual_seed(0)
    nn = torch.nn
    net = nn.Sequential(nn.Linear(eng.obs_dim, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, eng.action_dim)).to(DEV)
    log_std = torch.full((eng.action_dim,), -1.0, device=DEV)
    return net, log_std, MLPPolicy.from_torch(net, log_std=log_std)


def fixedwing_legs(n):
    eng = BatchEngine(build_params("fixedwing", "waypoints", seed=1), n, device=DEV)
    eng.env_reset()
    net, log_std, pol = nets(eng)
    std = log_std.exp()
    act = torch.zeros(n, 4, device=DEV)
    eps = torch.empty(n, 4, device=DEV)
    step = [0]

    def leg_s():
        eng.rollout_policy_steps(pol, K, step_index0=step[0])
        step[0] += K

    def leg_e():
        for _ in range(K):
            eng.env_step(act)

    def loop():
        with torch.no_grad():
            for _ in range(K):
                torch.addcmul(net(eng.obs), std, eps.normal_(), out=act)
                eng.env_step(act)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        loop()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loop()
    return {"S": leg_s, "E": leg_e, "C": loop, "D": g.replay}, [eng]


def hover_legs(n):
    engs = [BatchEngine(build_params("quadx", "hover", seed=1), n, device=DEV) for _ in range(2)]
    for e in engs:
        e.env_reset()
    pol = nets(engs[0])[2]
    step = [0, 0]

    def leg_f():
        engs[0].rollout_policy(pol, K, step_index0=step[0])
        step[0] += K

    def leg_s():
        engs[1].rollout_policy_steps(pol, K, step_index0=step[1])
        step[1] += K

    return {"F": leg_f, "S": leg_s}, engs


def act_legs(n):
    hover = BatchEngine(build_params("quadx", "hover", seed=1), n, device=DEV)
    dog = BatchEngine(build_params("fixedwing", "dogfight", seed=1, autoreset="off", angle_representation="euler", vehicle_options=dict(drone_model="acrowing"),
                                   dogfight=dict(team_size=4, assisted_flight=False)), n, device=DEV)
    legs = {}
    for name, eng in (("D21", hover), ("D123", dog)):
        eng.env_reset()
        pol = nets(eng)[2]
        out, mean = torch.empty(n, eng.action_dim, device=DEV), torch.empty(n, eng.action_dim, device=DEV)

        def leg(eng=eng, pol=pol, out=out, mean=mean):
            for s in range(K):
                eng.policy_act(pol, step_index=s, out=out, mean_out=mean)

        legs[name] = leg
    return legs, [hover, dog]


def floor_us(n, D, A):
    return 2.0 * n * (D * 64 + 64 * 64 + 64 * A) / (MATRIX_TF * 1e12) * 1e6 + LAUNCH_US


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
    return total * 1e3 / (reps * K)  # us per env step (per call for the act legs)


def run(make, n, repeats):
    legs, engs = make(n)
    samples = {name: [] for name in legs}
    for _ in range(repeats):
        for name, fn in legs.items():
            samples[name].append(time_leg(fn))
    del legs
    for e in engs:
        e.close()
    return {name: {"us": sorted(v)[len(v) // 2], "min": min(v), "max": max(v), "samples": v} for name, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536,524288")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parts", default="fixedwing,hover,act")
    args = ap.parse_args()
    res = {"workload": "64-64 tanh policy, Gaussian head, k = 100", "unit": "us per env step (act: us per call)", "sizes": {}}
    for n in (int(x) for x in args.sizes.split(",")):
        r = {}
        if "fixedwing" in args.parts:
            r["fixedwing_waypoints"] = run(fixedwing_legs, n, args.repeats)
        if "hover" in args.parts:
            r["hover"] = run(hover_legs, n, args.repeats)
        if "act" in args.parts:
            r["act"] = run(act_legs, n, args.repeats)
            for name, (D, A) in (("D21", (21, 4)), ("D123", (123, 6))):
                r["act"][name]["floor_us"] = floor_us(n, D, A)
                r["act"][name]["floor_share"] = r["act"][name]["floor_us"] / r["act"][name]["us"]
        res["sizes"][str(n)] = r
    line = json.dumps(res)
    print(line)
    if args.parts == "fixedwing,hover,act":
        os.makedirs(os.path.join(ROOT, "profiles", "policy_act"), exist_ok=True)
        open(os.path.join(ROOT, "profiles", "policy_act", "bench.json"), "w").write(line + "\n")


if __name__ == "__main__":
    main()

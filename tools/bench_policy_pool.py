"""What pf_policy_act_pool buys, and what its gather costs. 64-64 tanh policies with a Gaussian head throughout.

(a) microseconds per env step of the dogfight's closed loop against a pool of snapshots: 16 384 copies of 2 v 2 (65 536 aircraft),
    k = 64, 2 s episodes, env.rollout(policy, 64, opponent=[P snapshots]) with pooled=False (1 + P pf_policy_act over all rows and P
    merges per step: the code path as it was) and pooled=True (one pf_policy_act_pool), for P = 1, 4 and 16.
(b) microseconds per act call over 65 536 rows at D = 21 (Hover) and D = 123 (an eight-aircraft dogfight, six-wide actions), 100 calls
    per timed block, the library called directly on pf_policy blocks filled once (as the closed loops call it): pf_policy_act;
    pf_policy_act_pool with one policy; pf_policy_act_pool with 17 policies on equal contiguous segments.
(c) microseconds per pf_policy_pool_plan call at n = 65 536, P = 17 (equal segments), 20 calls per timed block.

Every leg runs on an env or engine of its own, in one process, on device events, each warmed up and timed over at least 0.5 s; the legs
of a group are alternated and repeated (default five times). Reported: median, min and max of the samples. The criterion of DESIGN.md
section 15 is evaluated for (a) at P = 4 and 16 -- the pooled median must lie below the unpooled one by more than the two legs' combined
min-max spread -- and printed as `clears_spread`; P = 1, (b) and (c) are recorded, not gated. Prints one JSON line and writes
profiles/policy_pool/bench.json.
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from pyflyt_amd import MLPPolicy, build_params  # noqa: E402
from pyflyt_amd import _lib as L  # noqa: E402
from pyflyt_amd.engine import BatchEngine  # noqa: E402
from pyflyt_amd.pz_envs import MAFixedwingDogfightEnv  # noqa: E402

K = 64
DEV = "cuda:0"
POOLS = (1, 4, 16)


def policy(D, A, seed):
    torch.manual_seed(seed)
    nn = torch.nn
    net = nn.Sequential(nn.Linear(D, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, A)).to(DEV)
    return MLPPolicy.from_torch(net, log_std=torch.full((A,), -1.0, device=DEV))


def loop_legs(num_envs):
    fns, envs = {}, []
    for P in POOLS:
        for pooled in (False, True):
            env = MAFixedwingDogfightEnv(team_size=2, num_envs=num_envs, seed=1, max_duration_seconds=2.0, device=DEV)
            env.reset(seed=1)
            eng = env.engine
            pol = policy(eng.obs_dim, eng.action_dim, 0)
            pool = [policy(eng.obs_dim, eng.action_dim, 1 + p) for p in range(P)]
            fns[f"pool{P}_{'pooled' if pooled else 'unpooled'}"] = (lambda env=env, pol=pol, pool=pool, pooled=pooled: env.rollout(pol, K, opponent=pool, pooled=pooled), K)
            envs.append(env)
    return fns, envs


def act_legs(n, calls=100):
    fns, engines, keep = {}, [], []
    for name, params in (("D21", build_params("quadx", "hover", seed=1)),
                         ("D123", build_params("fixedwing", "dogfight", seed=1, autoreset="off", angle_representation="euler",
                                               vehicle_options=dict(drone_model="acrowing"), dogfight=dict(team_size=4, assisted_flight=False)))):
        eng = BatchEngine(params, n, device=DEV)
        eng.env_reset()
        engines.append(eng)
        D, A = eng.obs_dim, eng.action_dim
        pols = [policy(D, A, p) for p in range(L.PF_POLICY_POOL_MAX)]
        out, obs = torch.empty(n, A, device=DEV), eng.obs
        plan1 = eng.policy_pool_plan(torch.zeros(n, dtype=torch.int32, device=DEV), 1)
        seg = (torch.arange(n, device=DEV) * L.PF_POLICY_POOL_MAX // n).to(torch.int32)
        plan17 = eng.policy_pool_plan(seg, L.PF_POLICY_POOL_MAX)

        def many(fn, calls=calls):
            def run():
                for s in range(calls):
                    fn(s)
            return run, calls

        # the blocks are filled once, as the closed loops do it: the legs time the launches, not the wrappers' 17 policy.fill() calls
        lib, ctx, stream = eng.lib, eng._ctx, eng._stream()
        one, many17 = eng._pool_blocks(pols[:1]), eng._pool_blocks(pols)
        q = eng._policy_block(pols[0])
        for block in (q, one[0], many17[0]):
            block.obs0 = obs.data_ptr()
        p_out, p1, p17 = C.c_void_p(out.data_ptr()), C.c_void_p(plan1.data_ptr()), C.c_void_p(plan17.data_ptr())
        keep.append((one, many17, q, plan1, plan17, out, pols))
        fns[f"{name}_policy_act"] = many(lambda s, q=q, p_out=p_out, lib=lib, ctx=ctx, stream=stream: L.check(lib.pf_policy_act(ctx, C.byref(q), p_out, s, stream), ctx))
        fns[f"{name}_pool_P1"] = many(lambda s, a=one, p=p1, nb=plan1.numel(), p_out=p_out, lib=lib, ctx=ctx, stream=stream:
                                      L.check(lib.pf_policy_act_pool(ctx, a, 1, p, nb, p_out, s, stream), ctx))
        fns[f"{name}_pool_P17"] = many(lambda s, a=many17, p=p17, nb=plan17.numel(), p_out=p_out, lib=lib, ctx=ctx, stream=stream:
                                       L.check(lib.pf_policy_act_pool(ctx, a, 17, p, nb, p_out, s, stream), ctx))
        if name == "D21":
            fns["plan_n65536_P17"] = many(lambda s, eng=eng, seg=seg: eng.policy_pool_plan(seg, L.PF_POLICY_POOL_MAX), 20)
    return fns, engines + [keep]


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
    return total * 1e3 / (reps * per)  # us per env step / per call


def measure(fns, repeats):
    samples = {name: [] for name in fns}
    for _ in range(repeats):
        for name, (fn, per) in fns.items():
            samples[name].append(time_leg(fn, per))
    return {name: {"us": sorted(v)[len(v) // 2], "min": min(v), "max": max(v), "samples": v} for name, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=16384)
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    res = {"workload": f"(a) team dogfight 2 v 2, {args.num_envs} copies ({4 * args.num_envs} aircraft), 64-64 tanh policies, Gaussian head, k = {K}, 60-step "
                       f"episodes, a pool of 1 / 4 / 16 snapshots; (b) one act over {args.rows} rows; (c) one plan over {args.rows} rows, 17 policies",
           "unit": "us per env step (a), us per call (b, c)"}
    fns, envs = loop_legs(args.num_envs)
    res["loop"] = measure(fns, args.repeats)
    for e in envs:
        e.close()
    del fns, envs
    torch.cuda.empty_cache()
    fns, engines = act_legs(args.rows)
    res["act"] = measure(fns, args.repeats)
    for e in engines[:-1]:
        e.close()
    res["clears_spread"] = {}
    for P in POOLS:
        u, p = res["loop"][f"pool{P}_unpooled"], res["loop"][f"pool{P}_pooled"]
        spread = (u["max"] - u["min"]) + (p["max"] - p["min"])
        res["clears_spread"][f"pool{P}"] = {"gain_us": u["us"] - p["us"], "combined_spread_us": spread, "clears": u["us"] - p["us"] > spread, "gated": P != 1}
    line = json.dumps(res)
    print(line)
    if args.num_envs == 16384 and args.rows == 65536:
        os.makedirs(os.path.join(ROOT, "profiles", "policy_pool"), exist_ok=True)
        open(os.path.join(ROOT, "profiles", "policy_pool", "bench.json"), "w").write(line + "\n")


if __name__ == "__main__":
    main()

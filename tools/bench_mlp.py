"""What pf_mlp_forward / pf_mlp_backward buy: one PPO epoch's network work with the networks through pyflyt_amd.mlp against the same
epoch through torch modules, D = 21, actor 64-64-4 tanh, critic 64-1 tanh.

  (a) epoch     ms per epoch = actor forward + critic forward + ppo_loss + backward() to every parameter's .grad
        M  through pyflyt_amd.mlp          (examples/10)
        T  through torch.nn.Sequential     (examples/08: what it replaces)
  (b) memory    torch.cuda.max_memory_allocated over one epoch of each leg, above what was allocated before it
  (c) calls     us per pf_mlp_forward and per pf_mlp_backward call of the actor alone, against FLOPs / 157.3 TF + 1.42 us per launch

One process, device events, every leg warmed up, at least 0.3 s per sample, the legs alternated, the median with min and max. Prints
one JSON line and writes profiles/mlp/bench.json.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import pyflyt_amd  # noqa: E402
from pyflyt_amd import build_params  # noqa: E402
from pyflyt_amd.engine import BatchEngine  # noqa: E402

DEV = "cuda:0"
D, A = 21, 4
MATRIX_TF, LAUNCH_US = 157.3, 1.42


def networks():
    torch.manual_seed(0)
    nn = torch.nn
    actor = nn.Sequential(nn.Linear(D, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, A)).to(DEV)
    critic = nn.Sequential(nn.Linear(D, 64), nn.Tanh(), nn.Linear(64, 1)).to(DEV)
    log_std = nn.Parameter(torch.full((A,), -0.5, device=DEV))
    return actor, critic, log_std


def batch(rows, actor, log_std):
    g = torch.Generator(device=DEV).manual_seed(1)
    o = torch.randn(rows, D, device=DEV, generator=g)
    with torch.no_grad():
        mean = torch.cat([actor(c) for c in o.split(1 << 18)])
        actions = mean + log_std.exp() * torch.randn(rows, A, device=DEV, generator=g)
        logp = torch.distributions.Normal(mean, log_std.exp()).log_prob(actions).sum(-1) - 0.05 * torch.randn(rows, device=DEV, generator=g)
        del mean
    adv, ret = torch.randn(rows, device=DEV, generator=g), torch.randn(rows, device=DEV, generator=g)
    valid = torch.rand(rows, device=DEV, generator=g) > 0.05
    return o, (actions, logp, adv, ret), valid


def epoch_legs(eng, rows):
    actor, critic, log_std = networks()
    o, b, valid = batch(rows, actor, log_std)
    params = list(actor.parameters()) + list(critic.parameters()) + [log_std]

    def epoch(fa, fc):
        loss, _ = pyflyt_amd.ppo_loss(eng, fa(o), log_std, fc(o), *b, valid=valid, clip=0.2, vf_coef=1.0, ent_coef=0.0, normalize_advantage=True)
        for p in params:
            p.grad = None
        loss.backward()

    return {"M": lambda: epoch(lambda x: pyflyt_amd.mlp(eng, x, actor), lambda x: pyflyt_amd.mlp(eng, x, critic)),
            "T": lambda: epoch(actor, critic)}


def call_legs(eng, rows):
    actor, _, _ = networks()
    layers = [(actor[i].weight.detach(), actor[i].bias.detach()) for i in (0, 2, 4)]
    g = torch.Generator(device=DEV).manual_seed(2)
    x, go = torch.randn(rows, D, device=DEV, generator=g), torch.randn(rows, A, device=DEV, generator=g)
    out = torch.empty(rows, A, device=DEV)
    return {"forward": lambda: eng.mlp_forward(x, layers, "tanh", out=out), "backward": lambda: eng.mlp_backward(x, go, layers, "tanh")}


def floors_us(rows):
    fwd = 2.0 * rows * (D * 64 + 64 * 64 + 64 * A)
    bwd = 2.0 * fwd + 2.0 * rows * (64 * 64 + 64 * A)  # the forward again, the three delta^T in products, delta W for the two hidden layers
    return {"forward": fwd / (MATRIX_TF * 1e12) * 1e6 + LAUNCH_US, "backward": bwd / (MATRIX_TF * 1e12) * 1e6 + 2.0 * LAUNCH_US}


def time_leg(fn, min_seconds=0.3):
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
    return total / reps  # ms per call


def peak_bytes(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_allocated(DEV)
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(DEV) - base


def measure(legs, repeats, scale=1.0):
    samples = {name: [] for name in legs}
    for _ in range(repeats):
        for name, fn in legs.items():
            samples[name].append(time_leg(fn) * scale)
    return {name: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v), "samples": v} for name, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default=f"{65536},{65536 * 64}")
    ap.add_argument("--epoch-rows", type=int, default=65536 * 64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp", "bench.json"))
    args = ap.parse_args()
    eng = BatchEngine(build_params("quadx", "none"), 64, device=DEV)
    res = {"workload": f"D = {D}, actor 64-64-{A} tanh, critic 64-1 tanh", "device": torch.cuda.get_device_name(0)}
    legs = epoch_legs(eng, args.epoch_rows)
    ep = measure(legs, args.repeats)
    spread = sum(v["max"] - v["min"] for v in ep.values())
    res["epoch"] = {"rows": args.epoch_rows, "unit": "ms per epoch", **ep, "combined_spread": spread,
                    "mlp_faster_by_more_than_the_spread": ep["T"]["median"] - ep["M"]["median"] > spread}
    res["peak_memory"] = {"unit": "bytes above the batch and the parameters", **{name: peak_bytes(fn) for name, fn in legs.items()}}
    del legs
    torch.cuda.empty_cache()
    res["calls"] = {"unit": "us per call (actor)"}
    for rows in (int(r) for r in args.rows.split(",")):
        c = measure(call_legs(eng, rows), args.repeats, scale=1e3)
        for name, f in floors_us(rows).items():
            c[name]["floor_us"] = f
            c[name]["floor_share"] = f / c[name]["median"]
        res["calls"][str(rows)] = c
    eng.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

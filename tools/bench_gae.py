"""What pf_gae buys: the post-processing of a 100-step closed-loop rollout (validity, GAE advantages and returns, log-probabilities).

  a  engine.gae(...)                           pf_gae alone: the scan kernel and the log-probability kernel
  b  the same quantities by a straightforward eager torch backward loop, written below: what a user writes today
  c  env.collect(policy, critic, 100)          end to end, beside
  r  env.rollout(policy, 100)                  the rollout alone

QuadX-Hover, 64-64 tanh policy with a Gaussian head, a 64-unit critic, k = 100, at 65 536 and 524 288 envs, NEXT_STEP and SAME_STEP.
One process, device events around batches of calls (at least 0.3 s per sample), every leg warmed up, the legs alternated and
repeated three times; median and spread. (a) and (b) are checked against each other before they are timed. Prints one JSON line and writes
profiles/gae/bench.json with the algorithmic bytes of pf_gae and the fraction of the 8 TB/s HBM peak they make at the time of (a).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from pyflyt_amd import MLPPolicy  # noqa: E402
from pyflyt_amd.gym_envs import make_vec  # noqa: E402

K, A = 100, 4
HBM_PEAK = 8.0e12  # bytes / s


def algorithmic_bytes(n, same_step):
    """Per lane-step: read reward 4, value 4, two flags 2, action 16, mean 16 (+ final value 4 under SAME_STEP); written advantage 4,
    return 4, log-probability 4, valid 1. Plus the last value row and, under NEXT_STEP, episode_start, once per lane."""
    per_step = 4 + 4 + 2 + 4 * A + 4 * A + (4 if same_step else 0) + 4 + 4 + 4 + 1
    return K * n * per_step + n * (4 + (0 if same_step else 1))


def torch_gae(same_step, gamma, lam, reward, term, trunc, values, final_values, episode_start, actions, mean, log_std):
    """The backward recursion a user writes in torch: selections by torch.where, one round of small kernels per step."""
    k = reward.shape[0]
    done = term | trunc
    if same_step:
        valid = torch.ones_like(done)
    else:
        valid = torch.cat([~episode_start[None], ~done[:-1]], 0)
    adv = torch.empty_like(reward)
    zero = torch.zeros_like(reward[0])
    nxt = zero
    for s in range(k - 1, -1, -1):
        nv = torch.where(done[s], final_values[s], values[s + 1]) if same_step else values[s + 1]
        delta = reward[s] + gamma * torch.where(term[s], zero, nv) - values[s]
        nxt = torch.where(valid[s], delta + gamma * lam * torch.where(done[s], zero, nxt), zero)
        adv[s] = nxt
    ret = adv + values[:-1]
    z = (actions - mean) * torch.exp(-log_std)
    logp = (-0.5 * z * z - log_std - 0.9189385332046727).sum(-1)
    return adv, ret, logp, valid


def make_legs(n, mode):
    env = make_vec("PyFlyt/QuadX-Hover-v4", n, seed=1, autoreset_mode=mode)
    env.reset()
    eng, dev = env.engine, env.device
    torch.manual_seed(0)
    nn = torch.nn
    net = nn.Sequential(nn.Linear(eng.obs_dim, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, A)).to(dev)
    critic = nn.Sequential(nn.Linear(eng.obs_dim, 64), nn.Tanh(), nn.Linear(64, 1)).to(dev)
    log_std = torch.full((A,), -1.0, device=dev)
    pol = MLPPolicy.from_torch(net, log_std=log_std)
    same = mode == "same_step"
    b = env.collect(pol, critic, K)  # a real trajectory for (a) and (b), copied out of the engine's buffers
    x = {key: b[key].clone() for key in ("reward", "terminated", "truncated", "actions", "mean")}
    x["values"] = torch.cat([b["values"], b["last_value"][None]], 0).contiguous()
    x["final_values"] = torch.randn(K, n, device=dev) if same else None
    x["episode_start"] = None if same else torch.zeros(n, dtype=torch.bool, device=dev)
    args = (x["reward"], x["terminated"], x["truncated"], x["values"])
    kw = dict(final_values=x["final_values"], episode_start=x["episode_start"], actions=x["actions"], mean=x["mean"], log_std=log_std)

    def leg_a():
        return eng.gae(*args, gamma=0.99, lam=0.95, **kw)

    def leg_b():
        return torch_gae(same, 0.99, 0.95, *args, x["final_values"], x["episode_start"], x["actions"], x["mean"], log_std)

    ours, theirs = leg_a(), leg_b()
    torch.cuda.synchronize()
    assert torch.equal(ours[3], theirs[3])
    for o, t in zip(ours[:3], theirs[:3]):
        assert (o - t).abs().max().item() < 1e-3, (o - t).abs().max().item()
    legs = {"a": leg_a, "b": leg_b, "c": lambda: env.collect(pol, critic, K), "r": lambda: env.rollout(pol, K)}
    return legs, env


def time_leg(fn, min_seconds=0.3):
    """us per call: batches of calls enqueued between ONE pair of device events (a call of tens of microseconds bracketed by its own
    events and a synchronise would time the host's launch and wake-up with it); the batch grows until it fills min_seconds."""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 4
    while True:
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        if ms >= min_seconds * 1e3 or reps >= 1 << 16:
            return ms * 1e3 / reps
        reps = max(reps * 2, int(reps * min_seconds * 1e3 / max(ms, 1e-3)) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="abcr")
    ap.add_argument("--sizes", default="65536,524288")
    ap.add_argument("--modes", default="next_step,same_step")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    res = {"workload": "QuadX-Hover, 64-64 tanh policy, Gaussian head, 64-unit critic, k = 100", "unit": "us per call", "hbm_peak_bytes_per_s": HBM_PEAK, "cases": {}}
    for n in (int(x) for x in args.sizes.split(",")):
        for mode in args.modes.split(","):
            legs, env = make_legs(n, mode)
            legs = {name: fn for name, fn in legs.items() if name in args.legs}
            samples = {name: [] for name in legs}
            for _ in range(args.repeats):
                for name, fn in legs.items():
                    samples[name].append(time_leg(fn))
            case = {name: {"us": sorted(v)[len(v) // 2], "min": min(v), "max": max(v), "samples": v} for name, v in samples.items()}
            if "a" in case:
                by = algorithmic_bytes(n, mode == "same_step")
                case["algorithmic_bytes"] = by
                case["hbm_fraction_of_peak"] = by / (case["a"]["us"] * 1e-6) / HBM_PEAK
                if "b" in case:
                    case["torch_over_pf_gae"] = case["b"]["us"] / case["a"]["us"]
            res["cases"][f"{n}/{mode}"] = case
            del legs
            env.close()
    line = json.dumps(res)
    print(line)
    if set(args.legs) == set("abcr"):
        os.makedirs(os.path.join(ROOT, "profiles", "gae"), exist_ok=True)
        open(os.path.join(ROOT, "profiles", "gae", "bench.json"), "w").write(line + "\n")


if __name__ == "__main__":
    main()

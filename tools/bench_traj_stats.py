"""What pf_traj_stats buys: the episode accounting and the normaliser moments of a 100-step closed-loop rollout.

  a  engine.traj_stats(..., obs=...)            pf_traj_stats alone: the scan, the observation-moments kernel and the finish kernel
  b  the same outputs by a straightforward eager torch loop, written below: what a user writes today
  c  env.collect(policy, critic, 100, stats=True)   end to end, beside
  d  env.collect(policy, critic, 100)               today's collect

QuadX-Hover (D = 21), 64-64 tanh policy with a Gaussian head, a 64-unit critic, k = 100, at 65 536 and 524 288 envs, NEXT_STEP and
SAME_STEP. One process, device events around batches of calls (at least 0.3 s per sample), every leg warmed up, the legs alternated
and repeated three times; median and spread. (a) and (b) are checked against each other before they are timed. Prints one JSON line
and writes profiles/traj_stats/bench.json with the algorithmic bytes of pf_traj_stats and the fraction of the 8 TB/s HBM peak they
make at the time of (a).

--masked: pf_traj_stats_masked against pf_traj_stats of the same library, on the NEXT_STEP trajectory above with pf_gae's valid_out as
the mask (so both compute the same bits, which is checked before they are timed), at the same shapes:

  a       engine.traj_stats(..., episode_start=..., obs=...)   pf_traj_stats
  m       engine.traj_stats(..., valid=..., obs=...)           pf_traj_stats_masked
  a_scan  (a) without obs: the scan and the finish kernel only
  m_scan  (m) without obs

Legs alternated and timed as above. Writes profiles/ma_stats/bench.json; no threshold, the numbers are recorded.
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
from tools.bench_gae import time_leg  # noqa: E402

K, A = 100, 4
HBM_PEAK = 8.0e12  # bytes / s


def algorithmic_bytes(n, D, next_step):
    """Per lane-step: read reward 4, two flags 2, the observation row 4 D; written episode return 4, episode length 4. Per lane: the
    three carries read and written, and episode_start under NEXT_STEP. (The observation kernel's second look at the flags under
    NEXT_STEP is not counted: it is the kernel's way, not the problem's.)"""
    return K * n * (4 + 2 + 4 * D + 4 + 4) + n * (24 + (1 if next_step else 0))


def torch_traj_stats(next_step, gamma, reward, term, trunc, episode_start, obs, carry, moments):
    """The forward recursion a user writes in torch: selections by torch.where, one round of small kernels per step; then the masked
    sums, and the moments of the batch merged into the running ones."""
    k = reward.shape[0]
    done = term | trunc
    valid = torch.cat([~episode_start[None], ~done[:-1]], 0) if next_step else torch.ones_like(done)
    ret, ln, G = carry
    ep_ret, ep_len, Gs = torch.empty_like(reward), torch.empty(reward.shape, dtype=torch.int32, device=reward.device), torch.empty_like(reward)
    zero, izero = torch.zeros_like(ret), torch.zeros_like(ln)
    for s in range(k):
        v = valid[s]
        ret = torch.where(v, ret + reward[s], ret)
        ln = torch.where(v, ln + 1, ln)
        G = torch.where(v, gamma * G + reward[s], G)
        Gs[s] = G
        fin = v & done[s]
        ep_ret[s] = torch.where(fin, ret, zero)
        ep_len[s] = torch.where(fin, ln, izero)
        ret, ln, G = torch.where(fin, zero, ret), torch.where(fin, izero, ln), torch.where(fin, zero, G)
    fin = valid & done
    r = ep_ret.double()
    inf = torch.full_like(r, float("inf"))
    summary = torch.stack([fin.sum().double(), r.sum(), (r * r).sum(), torch.where(fin, r, inf).min(), torch.where(fin, r, -inf).max(),
                           ep_len.sum().double(), (fin & term).sum().double(), (fin & ~term).sum().double()])
    out = []
    for x, (cnt, mean, m2) in ((Gs[..., None], moments[0]), (obs, moments[1])):
        w = valid[..., None]
        nb = valid.sum().double()
        d = torch.where(w, x - mean.float(), torch.zeros((), device=x.device))
        s1, s2 = d.sum((0, 1), dtype=torch.float64), (d * d).sum((0, 1), dtype=torch.float64)
        tot, delta = cnt + nb, s1 / nb
        out.append((tot, mean + delta * nb / tot, m2 + s2 - s1 * delta + delta * delta * cnt * nb / tot))
    return ep_ret, ep_len, summary, (ret, ln, G), out


def make_legs(n, mode):
    env = make_vec("PyFlyt/QuadX-Hover-v4", n, seed=1, autoreset_mode=mode)
    env.reset()
    eng, dev = env.engine, env.device
    torch.manual_seed(0)
    nn = torch.nn
    net = nn.Sequential(nn.Linear(eng.obs_dim, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, A)).to(dev)
    critic = nn.Sequential(nn.Linear(eng.obs_dim, 64), nn.Tanh(), nn.Linear(64, 1)).to(dev)
    pol = MLPPolicy.from_torch(net, log_std=torch.full((A,), -1.0, device=dev))
    nxt = mode == "next_step"
    b = env.collect(pol, critic, K)  # a real trajectory for (a) and (b), copied out of the engine's buffers
    x = {key: b[key].clone() for key in ("reward", "terminated", "truncated", "obs")}
    es = torch.zeros(n, dtype=torch.bool, device=dev) if nxt else None
    D = eng.obs_dim
    f64 = dict(dtype=torch.float64, device=dev)

    def leg_a():
        return eng.traj_stats(x["reward"], x["terminated"], x["truncated"], gamma=0.99, episode_start=es, obs=x["obs"])

    def leg_b():
        carry = (torch.zeros(n, device=dev), torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, device=dev))
        moments = ((torch.zeros((), **f64), torch.zeros(1, **f64), torch.zeros(1, **f64)), (torch.zeros((), **f64), torch.zeros(D, **f64), torch.zeros(D, **f64)))
        return torch_traj_stats(nxt, 0.99, x["reward"], x["terminated"], x["truncated"], es, x["obs"], carry, moments)

    ours, theirs = leg_a(), leg_b()
    torch.cuda.synchronize()
    assert torch.equal(ours[1], theirs[1]) and (ours[0] - theirs[0]).abs().max().item() < 1e-3
    assert torch.equal(ours[2][[0, 5, 6, 7]], theirs[2][[0, 5, 6, 7]]) and torch.allclose(ours[2], theirs[2], rtol=1e-6)
    # (the torch leg squares in float32 about a zero shift: its M2 = s2 - s1^2 / n is good to 1e-6 of s2 = M2 + n mean^2, not of M2)
    for ours_block, (cnt, mean, m2) in ((eng.obs_moments, theirs[4][1]), (eng.ret_moments, theirs[4][0])):
        w = mean.numel()
        assert ours_block[0] == cnt
        assert ((ours_block[1:1 + w] - mean).abs() <= 1e-5 * (mean.abs() + (m2 / cnt).sqrt()) + 1e-9).all()
        assert ((ours_block[1 + w:] - m2).abs() <= 1e-5 * (m2 + cnt * mean * mean) + 1e-9).all()
    legs = {"a": leg_a, "b": leg_b, "c": lambda: env.collect(pol, critic, K, stats=True), "d": lambda: env.collect(pol, critic, K)}
    return legs, env, dict(x, episode_start=es)


def make_masked_legs(n):
    _, env, x = make_legs(n, "next_step")  # (the trajectory of legs a and b)
    eng = env.engine
    valid = eng.gae(x["reward"], x["terminated"], x["truncated"], torch.zeros(K + 1, n, device=env.device), episode_start=x["episode_start"])[3].clone()
    flags = (x["reward"], x["terminated"], x["truncated"])

    def run(obs, **how):
        return eng.traj_stats(*flags, gamma=0.99, obs=obs, **how)

    masked = {"a": lambda: run(x["obs"], episode_start=x["episode_start"]), "m": lambda: run(x["obs"], valid=valid),
              "a_scan": lambda: run(None, episode_start=x["episode_start"]), "m_scan": lambda: run(None, valid=valid)}
    state = ("carry_return", "carry_length", "carry_disc", "obs_moments", "ret_moments")
    got = []
    for name in ("a", "m"):  # the same bits from both, from the empty state
        ts = eng._traj_state()
        for key in state:
            ts[key].zero_()
        out = masked[name]()
        got.append([t.clone() for t in out] + [ts[key].clone() for key in state])
    torch.cuda.synchronize()
    assert all(torch.equal(p.view(torch.uint8), q.view(torch.uint8)) for p, q in zip(*got))
    return masked, env, float(valid.float().mean())


def main_masked(args):
    res = {"workload": "pf_traj_stats_masked (m) against pf_traj_stats (a), QuadX-Hover (D = 21) NEXT_STEP trajectory, k = 100, valid = pf_gae's valid_out; "
                       "_scan: without obs (scan + finish only)", "unit": "us per call", "cases": {}}
    for n in (int(v) for v in args.sizes.split(",")):
        legs, env, share = make_masked_legs(n)
        samples = {name: [] for name in legs}
        for _ in range(args.repeats):
            for name, fn in legs.items():
                samples[name].append(time_leg(fn))
        case = {name: {"us": sorted(v)[len(v) // 2], "min": min(v), "max": max(v), "samples": v} for name, v in samples.items()}
        case["valid_share"] = share
        case["masked_over_unmasked"] = case["m"]["us"] / case["a"]["us"]
        case["masked_over_unmasked_scan"] = case["m_scan"]["us"] / case["a_scan"]["us"]
        res["cases"][f"{n}/next_step"] = case
        del legs
        env.close()
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles", "ma_stats"), exist_ok=True)
    open(os.path.join(ROOT, "profiles", "ma_stats", "bench.json"), "w").write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--masked", action="store_true", help="pf_traj_stats_masked against pf_traj_stats (see the module docstring)")
    ap.add_argument("--legs", default="abcd")
    ap.add_argument("--sizes", default="65536,524288")
    ap.add_argument("--modes", default="next_step,same_step")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if args.masked:
        return main_masked(args)
    res = {"workload": "QuadX-Hover (D = 21), 64-64 tanh policy, Gaussian head, 64-unit critic, k = 100", "unit": "us per call", "hbm_peak_bytes_per_s": HBM_PEAK,
           "cases": {}}
    for n in (int(x) for x in args.sizes.split(",")):
        for mode in args.modes.split(","):
            legs, env, _ = make_legs(n, mode)
            legs = {name: fn for name, fn in legs.items() if name in args.legs}
            samples = {name: [] for name in legs}
            for _ in range(args.repeats):
                for name, fn in legs.items():
                    samples[name].append(time_leg(fn))
            case = {name: {"us": sorted(v)[len(v) // 2], "min": min(v), "max": max(v), "samples": v} for name, v in samples.items()}
            if "a" in case:
                by = algorithmic_bytes(n, env.engine.obs_dim, mode == "next_step")
                case["algorithmic_bytes"] = by
                case["hbm_fraction_of_peak"] = by / (case["a"]["us"] * 1e-6) / HBM_PEAK
                if "b" in case:
                    case["torch_over_pf_traj_stats"] = case["b"]["us"] / case["a"]["us"]
            res["cases"][f"{n}/{mode}"] = case
            del legs
            env.close()
            torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if set(args.legs) == set("abcd"):
        os.makedirs(os.path.join(ROOT, "profiles", "traj_stats"), exist_ok=True)
        open(os.path.join(ROOT, "profiles", "traj_stats", "bench.json"), "w").write(line + "\n")


if __name__ == "__main__":
    main()

"""What pf_ppo_loss buys: the clipped PPO objective, its statistics and its gradients between the outputs of the actor and the critic
and their output-gradients.

  a  engine.ppo_loss(...)                      pf_ppo_loss alone: the advantage pass, the main kernel and the two finish kernels
  b  the same loss in eager torch float32 with backward() down to the gradients of mean, value and log_std: what a user writes today
  c  pyflyt_amd.ppo_loss(...) and backward()   (a) through the autograd wrapper, the grad_output multiply included
  o  engine.ppo_loss(..., clip_vf=, action_bounds=, bounds_coef=)   pf_ppo_loss_opt with both options on (only with --legs ao: what the
     options cost the pass; profiles/ppo_options/bench.json quotes it)

M = 65 536 x 64 and 524 288 x 64 rows, A = 4, a quarter of the rows invalid. One process, device events around batches of calls (at
least 0.3 s per sample), every leg warmed up, the legs alternated and repeated three times; median and spread. (a) and (b) are checked
against each other before they are timed. Prints one JSON line and writes profiles/ppo_loss/bench.json with the algorithmic bytes of
pf_ppo_loss and the fraction of the 8 TB/s HBM peak they make at the time of (a).
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import pyflyt_amd  # noqa: E402
from pyflyt_amd import build_params  # noqa: E402
from pyflyt_amd.engine import BatchEngine  # noqa: E402

A, CLIP, VF, ENT = 4, 0.2, 0.5, 0.01
HBM_PEAK = 8.0e12  # bytes / s
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def algorithmic_bytes(m):
    """Per row: the advantage pass reads the advantage 4 and the validity byte 1; the main kernel reads mean 16, action 16, old
    log-probability 4, advantage 4, return 4, value 4 and the validity byte 1, and writes grad_mean 16 and grad_value 4."""
    return m * ((4 + 1) + (4 * A + 4 * A + 4 + 4 + 4 + 4 + 1) + (4 * A + 4))


def torch_loss(mean, log_std, value, actions, logp_old, advantages, returns, valid):
    w = valid.float() / valid.sum()
    adv = advantages - (advantages * w).sum()
    adv = adv / (adv.pow(2) * w).sum().sqrt().clamp_min(1e-8)
    z = (actions - mean) * torch.exp(-log_std)
    logp = (-0.5 * z * z - log_std - HALF_LOG_2PI).sum(-1)
    ratio = (logp - logp_old).exp()
    surrogate = torch.minimum(ratio * adv, ratio.clamp(1 - CLIP, 1 + CLIP) * adv)
    value_loss = 0.5 * ((value - returns).pow(2) * w).sum()
    return -(surrogate * w).sum() + VF * value_loss - ENT * (log_std + (0.5 + HALF_LOG_2PI)).sum()


def make_legs(eng, m, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    r = dict(generator=g, device=dev)
    mean = torch.randn(m, A, **r).requires_grad_(True)
    log_std = torch.full((A,), -0.5, device=dev).requires_grad_(True)
    actions = (mean.detach() + torch.randn(m, A, **r) * log_std.detach().exp()).contiguous()
    z = (actions - mean.detach()) * torch.exp(-log_std.detach())
    # (the ratios sit at exp(d), d from five values well away from log(1 -+ clip): no row's branch is decided by float32 rounding, so
    #  (a) and (b) can be compared row by row)
    shifts = torch.tensor((-0.4, -0.1, 0.0, 0.1, 0.4), device=dev)[torch.randint(0, 5, (m,), **r)]
    logp_old = (-0.5 * z * z - log_std.detach() - HALF_LOG_2PI).sum(-1) - shifts
    advantages, returns = torch.randn(m, **r), torch.randn(m, **r) * 3.0
    value = (returns + torch.randn(m, **r)).requires_grad_(True)
    valid = torch.rand(m, **r) >= 0.25
    del z, shifts
    rest = (actions, logp_old, advantages, returns)
    kw = dict(clip=CLIP, vf_coef=VF, ent_coef=ENT, normalize_advantage=True)

    def leg_a():
        return eng.ppo_loss(mean.detach(), log_std.detach(), value.detach(), *rest, valid=valid, **kw)

    def leg_b():
        return torch.autograd.grad(torch_loss(mean, log_std, value, *rest, valid), [mean, value, log_std])

    values_old = value.detach() + 0.3 * (torch.arange(m, device=dev) % 3 == 0)  # (a third of the rows outside the clip range)
    opts = dict(clip_vf=0.2, values_old=values_old, action_bounds=([-1.0] * A, [1.0] * A), bounds_coef=1e-4)

    def leg_o():
        return eng.ppo_loss(mean.detach(), log_std.detach(), value.detach(), *rest, valid=valid, **kw, **opts)

    def leg_c():
        loss, _ = pyflyt_amd.ppo_loss(eng, mean, log_std, value, *rest, valid=valid, **kw)
        return torch.autograd.grad(loss, [mean, value, log_std])

    ours, theirs = leg_a(), leg_b()
    torch.cuda.synchronize()
    for o, t in zip(ours[:3], theirs):
        assert (o - t).abs().max().item() <= 1e-4 * max(t.abs().max().item(), 1e-12), ((o - t).abs().max().item(), t.abs().max().item())
    del ours, theirs
    return {"a": leg_a, "b": leg_b, "c": leg_c, "o": leg_o}


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
    ap.add_argument("--legs", default="abc")
    ap.add_argument("--envs", default="65536,524288")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    eng = BatchEngine(build_params("quadx", "none"), 64, device=dev)
    res = {"workload": f"pf_ppo_loss, A = {A}, M = envs x {args.steps} rows, a quarter invalid, normalised advantages", "unit": "us per call",
           "hbm_peak_bytes_per_s": HBM_PEAK, "cases": {}}
    for n in (int(x) for x in args.envs.split(",")):
        m = n * args.steps
        legs = {name: fn for name, fn in make_legs(eng, m, dev).items() if name in args.legs}
        samples = {name: [] for name in legs}
        for _ in range(args.repeats):
            for name, fn in legs.items():
                samples[name].append(time_leg(fn))
        case = {name: {"us": sorted(v)[len(v) // 2], "min": min(v), "max": max(v), "samples": v} for name, v in samples.items()}
        case["rows"] = m
        if "a" in case:
            by = algorithmic_bytes(m)
            case["algorithmic_bytes"] = by
            case["hbm_fraction_of_peak"] = by / (case["a"]["us"] * 1e-6) / HBM_PEAK
            if "b" in case:
                case["torch_over_pf_ppo_loss"] = case["b"]["us"] / case["a"]["us"]
            if "o" in case:
                case["options_over_pf_ppo_loss"] = case["o"]["us"] / case["a"]["us"]
        res["cases"][str(n)] = case
        del legs
        torch.cuda.empty_cache()
    eng.close()
    line = json.dumps(res)
    print(line)
    if set(args.legs) == set("abc") and args.envs == "65536,524288" and args.steps == 64:
        os.makedirs(os.path.join(ROOT, "profiles", "ppo_loss"), exist_ok=True)
        open(os.path.join(ROOT, "profiles", "ppo_loss", "bench.json"), "w").write(line + "\n")


if __name__ == "__main__":
    main()

"""What pf_adam_step buys: the optimiser's step of examples/10's PPO epoch (eleven tensors, 7 305 floats: actor 21-64-64-4, critic
21-64-1, log_std) with pyflyt_amd.Adam against torch.

  (a) step      us per step, global-norm clipping at 0.5 included, eager and again replayed from a captured graph
        P  pyflyt_amd.Adam(max_grad_norm=0.5).step()                                 (examples/11)
        F  clip_grad_norm_ + torch.optim.Adam, foreach (torch's default; capturable=True in the graph)
        U  the same with fused=True, where this torch build accepts it (the refusal is recorded otherwise)
  (b) epoch     ms per epoch of examples/10 (two mlp forwards, ppo_loss, backward(), clip + step) with torch's optimiser and with ours

One process, device events around INNER calls, every leg warmed up, at least 0.3 s per sample, the legs alternated, the median with
min and max. Prints one JSON line and writes profiles/adam/bench.json.
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
from tools.bench_mlp import DEV, batch, networks  # noqa: E402

MAX_NORM, LR = 0.5, 3e-4


def parameters():
    actor, critic, log_std = networks()
    return actor, critic, log_std, list(actor.parameters()) + list(critic.parameters()) + [log_std]


def step_legs(eng):
    """{name: (eager step, graph replay or the reason there is none)}; every leg owns its parameters and their fixed gradients."""
    legs = {}

    def add(name, make):
        params = parameters()[3]
        g = torch.Generator(device=DEV).manual_seed(3)
        for p in params:
            p.grad = torch.randn(p.shape, device=DEV, generator=g) * 0.1
        try:
            step, graph_step = make(params)
            for _ in range(3):
                step()
            torch.cuda.synchronize()
        except Exception as e:  # (a torch build that refuses fused=True on this device: said, not hidden)
            legs[name] = {"refused": f"{type(e).__name__}: {e}"[:300]}
            return
        try:
            for _ in range(3):
                graph_step()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                graph_step()
            replay = graph.replay
        except Exception as e:
            replay = f"{type(e).__name__}: {e}"[:300]
        legs[name] = {"eager": step, "graph": replay, "keep": params}

    def ours(params):
        opt = pyflyt_amd.Adam(eng, params, lr=LR, max_grad_norm=MAX_NORM)
        return opt.step, opt.step

    def torch_leg(**kw):
        def make(params):
            eager, cap = torch.optim.Adam(params, lr=LR, **kw), torch.optim.Adam(params, lr=LR, capturable=True, **kw)

            def step(opt):
                torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
                opt.step()
            return (lambda: step(eager)), (lambda: step(cap))
        return make

    add("P", ours)
    add("F", torch_leg(foreach=True))
    add("U", torch_leg(fused=True))
    return legs


def epoch_legs(eng, rows):
    out = {}
    for name in ("torch_optimiser", "pyflyt_amd_optimiser"):
        actor, critic, log_std, params = parameters()
        o, b, valid = batch(rows, actor, log_std)
        if name == "torch_optimiser":
            topt = torch.optim.Adam(params, lr=LR)

            def step(params=params, topt=topt):
                torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
                topt.step()
        else:
            step = pyflyt_amd.Adam(eng, params, lr=LR, max_grad_norm=MAX_NORM).step

        def epoch(actor=actor, critic=critic, log_std=log_std, params=params, o=o, b=b, valid=valid, step=step):
            loss, _ = pyflyt_amd.ppo_loss(eng, pyflyt_amd.mlp(eng, o, actor), log_std, pyflyt_amd.mlp(eng, o, critic), *b, valid=valid, clip=0.2, vf_coef=1.0,
                                          ent_coef=0.0, normalize_advantage=True)
            for p in params:
                p.grad = None
            loss.backward()
            step()
        out[name] = epoch
    return out


def kl_epoch_legs(eng, rows):
    """An epoch of examples/13 (ppo_grad and the step, on the engine's own tensors) with pf_adam_step, and with pf_kl_control +
    pf_adam_step_gated under a target no epoch reaches (the gate stays open: the same update), each eager and replayed from a
    captured graph: what the KL decisions cost when they are on the device (tools/bench_ppo_grad.py --options records it)."""
    out, keep = {}, []
    for name, kl in (("adam_step", {}), ("kl_control_and_gated_step", dict(target_kl=1e6, kl_stop=1.5))):
        actor, critic, log_std, params = parameters()
        o, (actions, logp, adv, ret), valid = batch(rows, actor, log_std)
        la = [(actor[i].weight.detach(), actor[i].bias.detach()) for i in (0, 2, 4)]
        lc = [(critic[i].weight.detach(), critic[i].bias.detach()) for i in (0, 2)]
        opt = pyflyt_amd.Adam(eng, [p.detach() for p in params], lr=LR, max_grad_norm=MAX_NORM, **kl)

        def epoch(o=o, la=la, lc=lc, ls=log_std.detach(), actions=actions, logp=logp, adv=adv, ret=ret, valid=valid, opt=opt, gated=bool(kl)):
            ga, gc, gls, stats = eng.ppo_grad(o, la, lc, ls, actions, logp, adv, ret, valid=valid, clip=0.2, vf_coef=1.0, ent_coef=0.0, normalize_advantage=True)
            grads = [t for pair in ga for t in pair] + [t for pair in gc for t in pair] + [gls]
            opt.step(grads=grads, stats=stats) if gated else opt.step(grads=grads)
        for _ in range(3):
            epoch()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            epoch()
        out[name], out[name + "_graph"] = epoch, graph.replay
        keep.append((graph, opt, params))
    return out, keep


def time_leg(fn, inner, min_seconds=0.3):
    """ms per call: device events around `inner` calls, repeated until min_seconds of them have been timed."""
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls, total = 0, 0.0
    while total < min_seconds * 1e3:
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        total += a.elapsed_time(b)
        calls += inner
    return total / calls


def measure(legs, repeats, inner, scale=1.0):
    samples = {name: [] for name in legs}
    for fn in legs.values():  # (one untimed sample of every leg: allocator, code objects and clocks settled before the first that counts)
        time_leg(fn, inner)
    for _ in range(repeats):
        for name, fn in legs.items():
            samples[name].append(time_leg(fn, inner) * scale)
    return {name: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v), "samples": v} for name, v in samples.items()}


def verdict(res):
    """section 15's criterion: P's median below the better torch leg's by more than the two legs' combined min-max spread"""
    rivals = {k: v for k, v in res.items() if k != "P" and "median" in v}
    if "P" not in res or not rivals:
        return None
    best = min(rivals, key=lambda k: rivals[k]["median"])
    spread = (res["P"]["max"] - res["P"]["min"]) + (rivals[best]["max"] - rivals[best]["min"])
    return {"better_torch_leg": best, "combined_spread": spread, "difference": rivals[best]["median"] - res["P"]["median"],
            "ours_faster_by_more_than_the_spread": rivals[best]["median"] - res["P"]["median"] > spread}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epoch-rows", default=f"{65536},{65536 * 64}")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam", "bench.json"))
    args = ap.parse_args()
    eng = BatchEngine(build_params("quadx", "none"), 64, device=DEV)
    res = {"workload": "examples/10's eleven tensors, 7 305 floats; clip at 0.5; Adam, lr 3e-4", "device": torch.cuda.get_device_name(0), "torch": torch.__version__}
    legs = step_legs(eng)
    res["step"] = {"unit": "us per step", "refused": {k: v["refused"] for k, v in legs.items() if "refused" in v}}
    for mode in ("eager", "graph"):
        run = {k: v[mode] for k, v in legs.items() if callable(v.get(mode))}
        m = measure(run, args.repeats, args.inner, scale=1e3)
        m.update({k: {"not_captured": v[mode]} for k, v in legs.items() if mode in v and not callable(v[mode])})
        m["verdict"] = verdict(m)
        res["step"][mode] = m
    del legs
    res["epoch"] = {"unit": "ms per epoch"}
    for rows in (int(r) for r in args.epoch_rows.split(",")):
        m = measure(epoch_legs(eng, rows), args.repeats, 4 if rows > (1 << 20) else 20)
        m["difference"] = m["torch_optimiser"]["median"] - m["pyflyt_amd_optimiser"]["median"]
        m["combined_spread"] = sum(v["max"] - v["min"] for v in m.values() if isinstance(v, dict))
        res["epoch"][str(rows)] = m
        torch.cuda.empty_cache()
    eng.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

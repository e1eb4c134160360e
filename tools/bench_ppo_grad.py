"""What pf_ppo_grad buys: one PPO epoch's gradients -- everything between the batch and every parameter's gradient tensor -- at
--epoch-rows rows, D = 21, actor 64-64-4 tanh, critic 64-1 tanh, through the engine's own calls (no autograd, no .grad bookkeeping:
the library's launches and their Python call overhead only).

  F  fused     BatchEngine.ppo_grad (pf_ppo_grad, seven launches)
  C  composed  mlp_forward x 2 -> ppo_loss -> mlp_backward x 2 of the same library (ten launches): the path it replaces

each eager and replayed from a captured graph (Fg, Cg); and the composed path's five calls one by one (`parts`: what the fused call's
two tile launches have to be set against). One process, device events, every leg warmed up, at least 0.3 s per sample,
the legs alternated, the median of --repeats with min and max. Also checks that both paths give the same network gradients bit for
bit, and records the intermediate tensors the composed path allocates. Prints one JSON line and writes profiles/ppo_grad/bench.json.

--options measures what PPO's options cost instead, and writes profiles/ppo_options/bench.json: pf_ppo_grad_opt with value clipping and
the bounds loss both on against pf_ppo_grad on the same rows (eager and replayed), and, through tools/bench_adam.py, an epoch with
pf_kl_control + pf_adam_step_gated against the same epoch with pf_adam_step.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from bench_mlp import A, D, DEV, batch, measure, networks  # noqa: E402
from pyflyt_amd import build_params  # noqa: E402
from pyflyt_amd.engine import BatchEngine  # noqa: E402

COEF = dict(clip=0.2, vf_coef=1.0, ent_coef=0.0, normalize_advantage=True)


def legs(eng, rows):
    actor, critic, log_std = networks()
    o, (actions, logp, adv, ret), valid = batch(rows, actor, log_std)
    la = [(actor[i].weight.detach(), actor[i].bias.detach()) for i in (0, 2, 4)]
    lc = [(critic[i].weight.detach(), critic[i].bias.detach()) for i in (0, 2)]
    ls = log_std.detach()
    mean, value = torch.empty(rows, A, device=DEV), torch.empty(rows, 1, device=DEV)

    def fused():
        return eng.ppo_grad(o, la, lc, ls, actions, logp, adv, ret, valid=valid, **COEF)

    def composed():
        eng.mlp_forward(o, la, "tanh", out=mean)
        eng.mlp_forward(o, lc, "tanh", out=value)
        gm, gv, gls, stats = eng.ppo_loss(mean, ls, value, actions, logp, adv, ret, valid=valid, **COEF)
        return eng.mlp_backward(o, gm, la, "tanh"), eng.mlp_backward(o, gv, lc, "tanh"), gls, stats

    ga, gc, gls_f, stats_f = fused()
    wa, wc, gls_c, stats_c = composed()
    torch.cuda.synchronize()
    same = all(torch.equal(u, v) for got, want in ((ga, wa), (gc, wc)) for pg, pw in zip(got, want) for u, v in zip(pg, pw))
    agree = {"network_gradients_bit_identical": same,
             "grad_log_std_max_abs_difference": float((gls_f - gls_c).abs().max()),
             "stats_max_abs_difference": float((stats_f[:9] - stats_c[:9]).abs().max())}
    graphs = {}
    for name, fn in (("Fg", fused), ("Cg", composed)):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        graphs[name] = g
    intermediates = 4 * (rows * A + rows) * 2  # mean, value, grad_mean, grad_value
    gm, gv = eng.ppo_loss(mean, ls, value, actions, logp, adv, ret, valid=valid, **COEF)[:2]
    parts = {"forward_actor": lambda: eng.mlp_forward(o, la, "tanh", out=mean), "forward_critic": lambda: eng.mlp_forward(o, lc, "tanh", out=value),
             "ppo_loss": lambda: eng.ppo_loss(mean, ls, value, actions, logp, adv, ret, valid=valid, **COEF),
             "backward_actor": lambda: eng.mlp_backward(o, gm, la, "tanh"), "backward_critic": lambda: eng.mlp_backward(o, gv, lc, "tanh")}
    return {"F": fused, "C": composed, "Fg": graphs["Fg"].replay, "Cg": graphs["Cg"].replay}, agree, intermediates, parts


def option_legs(eng, rows):
    """pf_ppo_grad and pf_ppo_grad_opt (clip_vf = 0.2 around values_old = the critic's values shifted by 0.3 on every third row; the
    box [-1, 1] with bounds_coef = 1e-4) on the same rows, eager and replayed."""
    actor, critic, log_std = networks()
    o, (actions, logp, adv, ret), valid = batch(rows, actor, log_std)
    la = [(actor[i].weight.detach(), actor[i].bias.detach()) for i in (0, 2, 4)]
    lc = [(critic[i].weight.detach(), critic[i].bias.detach()) for i in (0, 2)]
    ls = log_std.detach()
    values_old = eng.mlp_forward(o, lc, "tanh").reshape(-1).clone()
    values_old[::3] += 0.3
    opts = dict(clip_vf=0.2, values_old=values_old, action_bounds=([-1.0] * A, [1.0] * A), bounds_coef=1e-4)
    fns = {"plain": lambda: eng.ppo_grad(o, la, lc, ls, actions, logp, adv, ret, valid=valid, **COEF),
           "options": lambda: eng.ppo_grad(o, la, lc, ls, actions, logp, adv, ret, valid=valid, **COEF, **opts)}
    stats = fns["options"]()[3].clone()
    graphs = {}
    for name in ("plain", "options"):
        fns[name]()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fns[name]()
        graphs[name] = g
    fns.update({name + "_graph": g.replay for name, g in graphs.items()})
    return fns, graphs, {"value_clip_fraction": float(stats[12]), "bounds_loss": float(stats[13])}


def options_main(args):
    from bench_adam import kl_epoch_legs, measure as measure_inner

    eng = BatchEngine(build_params("quadx", "none"), 64, device=DEV)
    rows = args.epoch_rows
    res = {"workload": f"D = {D}, actor 64-64-{A} tanh, critic 64-1 tanh", "device": torch.cuda.get_device_name(0), "rows": rows}
    fns, graphs, seen = option_legs(eng, rows)
    t = measure(fns, args.repeats)
    g = {"unit": "ms per epoch of gradients", "options_on": "clip_vf 0.2, bounds_coef 1e-4 on [-1, 1]^4", **seen, **t}
    for a, b in (("options", "plain"), ("options_graph", "plain_graph")):
        g[f"{a}_against_{b}"] = {"difference_ms": t[a]["median"] - t[b]["median"], "ratio": t[a]["median"] / t[b]["median"],
                                 "combined_spread_ms": (t[a]["max"] - t[a]["min"]) + (t[b]["max"] - t[b]["min"])}
    res["ppo_grad_opt"] = g
    del fns, graphs
    res["kl_gate"] = {"unit": "ms per epoch (ppo_grad and the optimiser's step)"}
    for r in (65536, rows):
        legs, keep = kl_epoch_legs(eng, r)
        m = measure_inner(legs, args.repeats, 4 if r > (1 << 20) else 20)
        for a, b in (("kl_control_and_gated_step", "adam_step"), ("kl_control_and_gated_step_graph", "adam_step_graph")):
            m[f"{a}_minus_{b}_us"] = 1e3 * (m[a]["median"] - m[b]["median"])
        res["kl_gate"][str(r)] = m
        del legs, keep
        torch.cuda.empty_cache()
    eng.close()
    line = json.dumps(res)
    print(line)
    out = args.out if args.out_given else os.path.join(ROOT, "profiles", "ppo_options", "bench.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    open(out, "w").write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epoch-rows", type=int, default=65536 * 64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--options", action="store_true", help="time pf_ppo_grad_opt and the KL-gated step instead (profiles/ppo_options/bench.json)")
    args = ap.parse_args()
    args.out_given = args.out is not None
    if args.options:
        return options_main(args)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "ppo_grad", "bench.json")
    eng = BatchEngine(build_params("quadx", "none"), 64, device=DEV)
    res = {"workload": f"D = {D}, actor 64-64-{A} tanh, critic 64-1 tanh", "device": torch.cuda.get_device_name(0), "rows": args.epoch_rows,
           "unit": "ms per epoch of gradients", "launches": {"F": 7, "C": 10}}
    fns, agree, intermediates, parts = legs(eng, args.epoch_rows)
    t = measure(fns, args.repeats)
    res.update(t)
    res["parts"] = {"unit": "ms per call (composed path)", **{k: {q: v[q] for q in ("median", "min", "max")} for k, v in measure(parts, args.repeats).items()}}
    res["agreement"] = agree
    res["composed_intermediate_bytes"] = intermediates
    for f, c in (("F", "C"), ("Fg", "Cg")):
        spread = (t[f]["max"] - t[f]["min"]) + (t[c]["max"] - t[c]["min"])
        gain = t[c]["median"] - t[f]["median"]
        res[f"{f}_against_{c}"] = {"composed_minus_fused_ms": gain, "combined_spread_ms": spread, "fused_over_composed": t[f]["median"] / t[c]["median"],
                                   "verdict": "faster" if gain > spread else "slower" if -gain > spread else "within the spread"}
    del fns, parts
    eng.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

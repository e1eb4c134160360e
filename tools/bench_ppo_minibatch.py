"""What pf_ppo_grad_rows buys: one PPO epoch of shuffled minibatches over a batch of --rows rows (5 % of them invalid), D = 21, actor
64-64-4 tanh, critic 64-1 tanh, value clipping on (so that all seven per-row tensors are read), through the engine's own calls. Per
minibatch count (4 and 32), three legs, each timed per EPOCH, that is as the sum over its minibatches of one seeded permutation:

  a  gather   what the library allowed before: torch.index_select of the seven per-row tensors into buffers that are reused from
              minibatch to minibatch (no allocation inside the leg), then BatchEngine.ppo_grad on the copies
  b  rows     BatchEngine.ppo_grad(rows=idx): nothing is gathered
  c  slice    BatchEngine.ppo_grad on a contiguous slice of m rows: the floor, no shuffle at all; b - c is the cost of the indirection

One process, device events, every leg warmed up, at least 0.3 s per sample, the legs alternated, the median of --repeats with min and
max. Also checks that a and b give the same bits, and records the bytes leg a keeps resident for its copies. Prints one JSON line and
writes profiles/ppo_grad_rows/bench.json.
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

COEF = dict(clip=0.2, vf_coef=1.0, ent_coef=0.0, normalize_advantage=True, clip_vf=0.2)


def legs(eng, data, perm, count):
    """The three legs of an epoch of `count` minibatches, what they agree on, and the bytes of leg a's copies."""
    la, lc, ls, tensors = data
    names = ("x", "actions", "logp_old", "advantages", "returns", "valid", "values_old")
    parts = list(torch.tensor_split(perm, count))
    m = max(p.numel() for p in parts)
    bufs = {k: torch.empty((m, *tensors[k].shape[1:]), dtype=tensors[k].dtype, device=DEV) for k in names}

    def grad(t, rows=None):
        return eng.ppo_grad(t["x"], la, lc, ls, t["actions"], t["logp_old"], t["advantages"], t["returns"], valid=t["valid"], values_old=t["values_old"],
                            rows=rows, **COEF)

    def gather(idx):
        n = idx.numel()
        views = {k: bufs[k][:n] for k in names}
        for k in names:
            torch.index_select(tensors[k], 0, idx, out=views[k])
        return views

    def leg_a():
        for idx in parts:
            grad(gather(idx))

    def leg_b():
        for idx in parts:
            grad(tensors, rows=idx)

    def leg_c():
        lo = 0
        for idx in parts:
            grad({k: tensors[k][lo:lo + idx.numel()] for k in names})
            lo += idx.numel()

    def outputs(o):
        ga, gc, gls, stats = o
        return [t.clone() for net in (ga, gc) for pair in net for t in pair] + [gls.clone(), stats.clone().view(torch.int64)]

    want, got = outputs(grad(gather(parts[-1]))), outputs(grad(tensors, rows=parts[-1]))
    torch.cuda.synchronize()
    agree = all(torch.equal(u, v) for u, v in zip(want, got))
    return {"a_gather": leg_a, "b_rows": leg_b, "c_slice": leg_c}, agree, sum(b.numel() * b.element_size() for b in bufs.values()), m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536 * 64)
    ap.add_argument("--minibatches", default="4,32")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_grad_rows", "bench.json"))
    args = ap.parse_args()
    eng = BatchEngine(build_params("quadx", "none"), 64, device=DEV)
    actor, critic, log_std = networks()
    o, (actions, logp, adv, ret), valid = batch(args.rows, actor, log_std)
    la = [(actor[i].weight.detach(), actor[i].bias.detach()) for i in (0, 2, 4)]
    lc = [(critic[i].weight.detach(), critic[i].bias.detach()) for i in (0, 2)]
    values_old = torch.cat([eng.mlp_forward(c, lc, "tanh").reshape(-1).clone() for c in o.split(1 << 20)])
    values_old[::3] += 0.3
    tensors = dict(x=o, actions=actions, logp_old=logp, advantages=adv, returns=ret, valid=valid, values_old=values_old)
    perm = torch.randperm(args.rows, dtype=torch.int32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    res = {"workload": f"D = {D}, actor 64-64-{A} tanh, critic 64-1 tanh, clip_vf 0.2", "device": torch.cuda.get_device_name(0), "rows_total": args.rows,
           "valid_fraction": float(valid.float().mean()), "unit": "ms per epoch (the sum over the epoch's minibatches)", "minibatches": {}}
    for count in (int(c) for c in args.minibatches.split(",")):
        fns, agree, copy_bytes, m = legs(eng, (la, lc, log_std.detach(), tensors), perm, count)
        t = measure(fns, args.repeats)
        r = {"m": m, **t, "a_and_b_bit_identical": agree, "a_extra_resident_bytes": copy_bytes}
        spread = lambda p, q: (t[p]["max"] - t[p]["min"]) + (t[q]["max"] - t[q]["min"])  # noqa: E731
        gain = t["a_gather"]["median"] - t["b_rows"]["median"]
        r["b_against_a"] = {"gather_minus_rows_ms": gain, "combined_spread_ms": spread("a_gather", "b_rows"), "rows_over_gather": t["b_rows"]["median"] / t["a_gather"]["median"],
                            "verdict": "faster" if gain > spread("a_gather", "b_rows") else "slower" if -gain > spread("a_gather", "b_rows") else "within the spread"}
        r["indirection"] = {"rows_minus_slice_ms": t["b_rows"]["median"] - t["c_slice"]["median"], "gathers_cost_ms": t["a_gather"]["median"] - t["c_slice"]["median"],
                            "combined_spread_ms": spread("b_rows", "c_slice")}
        res["minibatches"][str(count)] = r
        del fns
        torch.cuda.empty_cache()
    eng.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

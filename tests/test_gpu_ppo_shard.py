"""The sharded PPO gradient on the device: pf_ppo_adv_sums, pf_adv_sums_add, pf_ppo_grad_shard, pf_ppo_shard_combine, pf_moments_merge,
their BatchEngine methods and pyflyt_amd.ppo_grad_sharded, on one context (shards are then slices of one batch on one device).

1. One shard is today's call: adv_sums -> grad_shard -> combine gives ppo_grad's bits, every output (fails without the feature).
2. The combine is exact: grad_out is the float32 rounding of the float64 sum of the shard buffers, added in ascending order.
3. Shards give the joint gradient: against float64 autograd on the whole batch with the project's tolerance for pf_ppo_grad per shard
   plus one rounding of the combine, and against the single call on the concatenated batch (order-free slots equal, summed slots
   within test_gpu_ppo_grad.py's reorder_bounds).
4. Garbage in unselected rows reaches nothing.   5. Determinism: a second stream, repetition, a captured graph of the whole call.
6. pf_moments_merge against Chan's formula in float64.   7. The raw ABI's refusals.

Shapes: test_gpu_ppo_grad.py's (1, 63 / 64 / 65: the ragged tile; 129; 64 * 256 + 1: a second tile per workgroup), its networks and batch."""
import copy
import ctypes as C
import math

import pytest
import torch

import pyflyt_amd
from pyflyt_amd import PyFlytAmdError, build_params
from pyflyt_amd import _lib as L
from pyflyt_amd.engine import BatchEngine
from test_gpu_ppo_grad import COEF, DEV, NETS, STRIDE, U64, case, cpu_gradients, layers_of, on_device, params_of, reorder_bounds, written_out_loss
from test_gpu_ppo_loss import HALF_LOG_2PI, f32

pytestmark = pytest.mark.gpu
BOUNDS_COEF = 0.0078125
BATCH_KEYS = ("x", "actions", "logp_old", "advantages", "returns", "valid", "values_old")


@pytest.fixture(scope="module")
def eng():
    e = BatchEngine(build_params("quadx", "none"), 64, device=DEV)  # (a context WITHOUT an env task: any context serves)
    yield e
    e.close()


def with_options(c):
    """The case with values_old (the returns moved by up to 0.6: rows on both sides of clip_vf = 0.2) for the calls with options."""
    g = torch.Generator().manual_seed(5 + c["x"].shape[0])
    return dict(c, values_old=(c["returns"].double() + (torch.rand(c["x"].shape[0], generator=g, dtype=torch.float64) - 0.5) * 1.2).float())


def options_of(b, A):
    return dict(clip_vf=0.2, values_old=b["values_old"], action_bounds=([-0.25] * A, [0.25] * A), bounds_coef=BOUNDS_COEF)


def to_device(c):
    actor, critic, log_std, b = on_device(c)
    if c.get("values_old") is not None:
        b["values_old"] = c["values_old"].to(DEV)
    return actor, critic, log_std, b


def single_call(eng, actor, critic, log_std, b, activation, rows=None, opts=None, coef=COEF):
    """(flat gradient, grad_log_std, stats) of BatchEngine.ppo_grad, as copies, the gradients in the flat layout of the sharded calls."""
    ga, gc, gls, stats = eng.ppo_grad(b["x"], layers_of(actor), layers_of(critic), log_std.detach(), b["actions"], b["logp_old"], b["advantages"],
                                      b["returns"], valid=b["valid"], actor_activation=activation, critic_activation=activation, rows=rows, **coef, **(opts or {}))
    return torch.cat([t.reshape(-1) for net in (ga, gc) for pair in net for t in pair]), gls.clone(), stats.clone()


def sharded_call(eng, actor, critic, log_std, shards, activation, opts=None, coef=COEF):
    """The four steps on one context. shards: [(b, rows or None)], b a batch dict of device tensors. Returns (flat gradient,
    grad_log_std, stats, the shards' flats, blocks, the global sums), as copies."""
    A = log_std.numel()
    sums = [eng.ppo_adv_sums(b["advantages"], valid=b["valid"], rows=rows).clone() for b, rows in shards]
    total = eng.adv_sums_add(sums).clone()
    flats, blocks = [], []
    for b, rows in shards:
        o = {} if opts is None else options_of(b, A)
        _, _, flat, block = eng.ppo_grad_shard(b["x"], layers_of(actor), layers_of(critic), log_std.detach(), b["actions"], b["logp_old"], b["advantages"],
                                               b["returns"], total, valid=b["valid"], actor_activation=activation, critic_activation=activation, rows=rows,
                                               **coef, **o)
        flats.append(flat.clone())
        blocks.append(block.clone())
    grad, gls, stats = eng.ppo_shard_combine(blocks, total, flats, log_std.detach(), vf_coef=coef["vf_coef"], ent_coef=coef["ent_coef"],
                                             value_clip=opts is not None, bounds_coef=BOUNDS_COEF if opts is not None else 0.0)
    return grad.clone(), gls.clone(), stats.clone(), flats, blocks, total


def same_bits(a, b):
    return torch.equal(a, b) or bool(((a == b) | (a.isnan() & b.isnan())).all())


def index_list(rows, seed, out_of_range=True):
    """A shuffled index list over `rows` rows with a duplicate and, with out_of_range, the numbers -1 and `rows` in it."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randperm(rows, generator=g, dtype=torch.int32)
    extra = [int(idx[0])] + ([-1, rows] if out_of_range else [])
    idx = torch.cat([idx, torch.tensor(extra, dtype=torch.int32)])
    return idx[torch.randperm(idx.numel(), generator=g)].contiguous().to(DEV)


# ---------------------------------------------------------------------------------------------- 1. one shard is today's call
@pytest.mark.parametrize("rows", [1, 63, 64, 65, STRIDE])
@pytest.mark.parametrize("indexed", [False, True])
@pytest.mark.parametrize("options", [False, True])
def test_one_shard_has_the_bits_of_ppo_grad(eng, rows, indexed, options):
    for net in (0, 1) if rows in (65, STRIDE) else (0,):  # (four wide and tanh; seven wide, ReLU, a three-layer critic)
        c = with_options(case(rows, net, "quarter"))
        actor, critic, log_std, b = to_device(c)
        idx = index_list(rows, 3 * rows + net) if indexed else None
        opts = options_of(b, log_std.numel()) if options else None
        want = single_call(eng, actor, critic, log_std, b, c["activation"], rows=idx, opts=opts)
        got = sharded_call(eng, actor, critic, log_std, [(b, idx)], c["activation"], opts=opts)
        assert torch.equal(got[0], want[0]), float((got[0] - want[0]).abs().max())  # every network gradient
        assert torch.equal(got[1], want[1])  # grad_log_std
        assert same_bits(got[2], want[2]), (got[2].tolist(), want[2].tolist())  # all 16 slots (slot 9 is NaN on one row)
        assert float(got[2][14]) == (2.0 if indexed else 0.0) and float(got[0].abs().max()) > 0
        assert torch.equal(got[3][0], want[0])  # (one shard's share is the whole gradient: the combine's sum is a copy)
        block = got[4][0].tolist()
        assert block[20] == float(want[2][0]) and block[21] == float(want[2][14]) and block[22:] == [0.0, 0.0]
        if not options:
            assert block[17:20] == [0.0, 0.0, 0.0]
        assert block[9 + log_std.numel():17] == [0.0] * (8 - log_std.numel())


# ---------------------------------------------------------------------------------------------- 2. the combine is exact
def cut(c, bounds):
    """The case's batch in contiguous slices [bounds[g], bounds[g + 1])."""
    return [dict(c, **{k: (None if c.get(k) is None else c[k][lo:hi].contiguous()) for k in BATCH_KEYS}) for lo, hi in zip(bounds[:-1], bounds[1:])]


def shards_on_device(parts):
    return [{k: (None if p.get(k) is None else p[k].to(DEV)) for k in BATCH_KEYS} for p in parts]


@pytest.mark.parametrize("rows, bounds", [(129, [0, 100, 129]), (STRIDE, [0, 5000, 5063, STRIDE]), (16, list(range(17)))])
def test_combine_is_the_rounded_double_sum_in_shard_order(eng, rows, bounds):
    c = case(rows, 0, "quarter")
    actor, critic, log_std, _ = on_device(c)
    shards = [(b, None) for b in shards_on_device(cut(c, bounds))]
    grad, _, stats, flats, blocks, total = sharded_call(eng, actor, critic, log_std, shards, c["activation"])
    assert len(flats) == len(bounds) - 1
    acc = flats[0].double().cpu()
    for f in flats[1:]:
        acc = acc + f.double().cpu()
    assert torch.equal(grad.cpu(), acc.float())
    assert float(stats[0]) == float(c["valid"].sum()) == sum(float(b[20]) for b in blocks) == float(total[0])
    for g, ((b, _), blk) in enumerate(zip(shards, blocks)):
        assert float(blk[20]) == float(b["valid"].sum()), g


# ---------------------------------------------------------------------------------------------- 3. shards give the joint gradient
def shard_loss(actor, critic, log_std, c, dtype, coef, keep):
    """test_gpu_ppo_grad.py's written_out_loss restricted to the rows of `keep` under the GLOBAL c, mu and sigma (those of all valid
    rows of c), without the entropy term (which belongs to no shard: its gradient is the constant -ent_coef)."""
    clip, vf_coef = f32(coef["clip"]), f32(coef["vf_coef"])
    M = c["x"].shape[0]
    v = torch.ones(M, dtype=torch.bool) if c["valid"] is None else c["valid"]
    cnt = int(v.sum())
    w = 1.0 / cnt if cnt else 0.0
    zero = torch.zeros((), dtype=dtype)
    a64 = c["advantages"].double()
    mu = float(torch.where(v, a64, 0.0).sum()) * w
    sigma = math.sqrt(float(torch.where(v, (a64 - mu) ** 2, 0.0).sum()) * w)
    adv = c["advantages"].to(dtype)
    a = (adv - f32(mu)) * f32(1.0 / max(sigma, 1e-8)) if coef["normalize_advantage"] else adv
    x = c["x"].to(dtype)
    mean, value = actor(x), critic(x).squeeze(-1)
    z = (c["actions"].to(dtype) - mean) * torch.exp(-log_std)
    logp = (-0.5 * z * z - log_std - HALF_LOG_2PI).sum(-1)
    r = torch.exp(logp - c["logp_old"].to(dtype))
    surr = torch.minimum(r * a, torch.clamp(r, 1.0 - clip, 1.0 + clip) * a)
    wt = torch.tensor(w, dtype=dtype)
    live = v & keep
    policy_loss = -(torch.where(live, surr, zero).sum() * wt)
    value_loss = 0.5 * (torch.where(live, (value - c["returns"].to(dtype)) ** 2, zero).sum() * wt)
    return policy_loss + vf_coef * value_loss, mu, sigma


def shard_gradients(c, dtype, coef, keep):
    actor, critic = copy.deepcopy(c["actor"]).to(dtype), copy.deepcopy(c["critic"]).to(dtype)
    log_std = torch.nn.Parameter(c["log_std"].to(dtype))
    shard_loss(actor, critic, log_std, c, dtype, coef, keep)[0].backward()
    return [torch.zeros_like(p, dtype=torch.float64) if p.grad is None else p.grad.double() for p in params_of(actor, critic, log_std)]


def far_from_a_float32_boundary(v):
    """|v - the nearest midpoint of two neighbouring float32s| >= 2^-40 |v|: float32(v) is the same however v's last bits fall."""
    f = torch.tensor(v, dtype=torch.float64).float()
    mids = [(f.double() + torch.nextafter(f, torch.tensor(s * math.inf)).double()) / 2.0 for s in (-1.0, 1.0)]
    return min(abs(float(m) - v) for m in mids) >= 2.0 ** -40 * abs(v)


# (the cuts and the shard without a valid row were chosen on the CPU: with [0, 20, 65] the 32 valid rows left put mu exactly on the
#  midpoint of two float32s, where the last bit of a double sum decides its rounding)
JOINT = [(65, 0, [0, 21, 65], 0), (65, 1, [0, 1, 40, 65], 1), (129, 0, [0, 64, 129], 1), (129, 4, [0, 30, 31, 129], 1),
         (STRIDE, 0, [0, 7000, STRIDE], 0), (STRIDE, 2, [0, 100, 9000, STRIDE], 1)]  # rows, net, the cuts, the shard without a valid row


@pytest.mark.parametrize("rows, net, bounds, empty", JOINT)
def test_shards_give_the_gradient_of_the_joint_batch(eng, rows, net, bounds, empty):
    c = dict(case(rows, net, "quarter"))
    G = len(bounds) - 1
    c["valid"] = c["valid"].clone()
    c["valid"][bounds[empty]:bounds[empty + 1]] = False  # one shard has no valid row
    actor, critic, log_std, b = on_device(c)
    # the last shard goes through a shuffled index list with a duplicate-free permutation and one number outside its rows
    parts = shards_on_device(cut(c, bounds))
    last = bounds[-1] - bounds[-2]
    gen = torch.Generator().manual_seed(rows + net)
    perm = torch.randperm(last, generator=gen, dtype=torch.int32)
    idx_last = torch.cat([perm[: last // 2], torch.tensor([last], dtype=torch.int32), perm[last // 2:]]).contiguous()
    shards = [(p, None) for p in parts[:-1]] + [(parts[-1], idx_last.to(DEV))]
    grad, gls, stats, flats, blocks, total = sharded_call(eng, actor, critic, log_std, shards, c["activation"])
    assert float(blocks[empty][20]) == 0.0 and not bool(flats[empty].any()) and float(blocks[-1][21]) == 1.0

    # (a) float64 autograd on the whole batch; the tolerance of pf_ppo_grad per shard, and one rounding of the combine
    g64 = cpu_gradients(c, torch.float64, COEF)
    keeps = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        k = torch.zeros(rows, dtype=torch.bool)
        k[lo:hi] = True
        keeps.append(k)
    ref_g = [shard_gradients(c, torch.float64, COEF, k) for k in keeps]
    e32_g = [shard_gradients(c, torch.float32, COEF, k) for k in keeps]
    whole = written_out_loss(copy.deepcopy(c["actor"]).double(), copy.deepcopy(c["critic"]).double(), c["log_std"].double(), c, torch.float64, COEF)
    parts64 = sum(shard_loss(copy.deepcopy(c["actor"]).double(), copy.deepcopy(c["critic"]).double(), c["log_std"].double(), c, torch.float64, COEF, k)[0] for k in keeps)
    H = float((c["log_std"].double() + (0.5 + HALF_LOG_2PI)).sum())
    assert abs(float(whole) - (float(parts64) - f32(COEF["ent_coef"]) * H)) <= 1e-12 * max(1.0, abs(float(whole)))  # (the shard losses are the whole's)
    names = [f"actor.{n}" for n, _ in actor.named_parameters()] + [f"critic.{n}" for n, _ in critic.named_parameters()] + ["log_std"]
    got, at = [], 0
    for p in params_of(actor, critic, log_std)[:-1]:
        got.append(grad[at:at + p.numel()].view(p.shape))
        at += p.numel()
    got.append(gls)
    ratios = {}
    for i, (name, g, ref) in enumerate(zip(names, got, g64)):
        bound = sum(8.0 * max(float((e32_g[s][i] - ref_g[s][i]).abs().max()), 2.0 ** -24 * float(ref_g[s][i].abs().max())) for s in range(G))
        bound += 2.0 ** -24 * float(ref.abs().max())
        ratios[name] = float((g.double().cpu() - ref).abs().max()) / max(bound, 1e-300)
    print(f"rows {rows} net {NETS[net]} cuts {bounds}: err / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    for k, v in ratios.items():
        assert v <= 1.0, (k, v)

    # (b) the single call on the concatenated batch, through the concatenated index lists (so that slot 14 counts the same slot)
    v64, a64 = c["valid"], c["advantages"].double()
    cnt = float(v64.sum())
    mu = float(torch.where(v64, a64, 0.0).sum()) / cnt
    sigma = math.sqrt(float(torch.where(v64, (a64 - mu) ** 2, 0.0).sum()) / cnt)
    assert far_from_a_float32_boundary(mu) and far_from_a_float32_boundary(1.0 / max(sigma, 1e-8))  # (chosen on the CPU: holds by construction)
    joint_idx = torch.cat([torch.arange(bounds[-2], dtype=torch.int32), torch.where(idx_last < last, idx_last + bounds[-2], -1)]).contiguous().to(DEV)
    want_grad, want_gls, want_stats = single_call(eng, actor, critic, log_std, b, c["activation"], rows=joint_idx)
    assert f32(float(stats[7])) == f32(float(want_stats[7])) == f32(mu)
    assert f32(1.0 / max(float(stats[8]), 1e-8)) == f32(1.0 / max(float(want_stats[8]), 1e-8)) == f32(1.0 / max(sigma, 1e-8))
    gs, ws = stats.tolist(), want_stats.tolist()
    for slot in (0, 6, 10, 11, 12, 14):
        assert gs[slot] == ws[slot], (slot, gs[slot], ws[slot])
    assert gs[14] == 1.0 and gs[0] == cnt
    with torch.no_grad():
        mean, value = pyflyt_amd.mlp(eng, b["x"], actor), pyflyt_amd.mlp(eng, b["x"], critic)
    bound, gb = reorder_bounds(b, log_std, mean, value, want_stats, COEF)
    line = []
    for slot in (1, 2, 3, 5, 9, 13):
        line.append(f"stats[{slot}] {abs(gs[slot] - ws[slot]):.2e} <= {bound[slot]:.2e}")
        assert abs(gs[slot] - ws[slot]) <= bound[slot], (slot, gs[slot], ws[slot], bound[slot])
    for cix, (g, w) in enumerate(zip(gls.tolist(), want_gls.tolist())):
        lim = gb[cix] + 2.0 ** -23 * abs(w)
        line.append(f"gls[{cix}] {abs(g - w):.2e} <= {lim:.2e}")
        assert abs(g - w) <= lim, (cix, g, w, lim)
    print("  against the single call: " + ", ".join(line))


# ---------------------------------------------------------------------------------------------- 4. garbage in unselected rows
def test_unselected_rows_reach_no_output(eng):
    rows, bounds = 129, [0, 64, 129]
    c = case(rows, 0, "quarter")
    actor, critic, log_std, _ = on_device(c)
    parts = shards_on_device(cut(c, bounds))
    named = torch.arange(0, 65, 2, dtype=torch.int32, device=DEV)  # the second shard's even rows: the odd ones are named by no index

    def run(ps):
        return sharded_call(eng, actor, critic, log_std, [(ps[0], None), (ps[1], named)], c["activation"])[:3]

    clean = run(parts)
    dirty = [dict(p) for p in parts]
    for g, p in enumerate(dirty):
        bad = ~p["valid"]
        if g == 1:
            bad = bad.clone()
            bad[1::2] = True
            p["x"] = p["x"].clone()
            p["x"][1::2] = float("nan")  # (a row no index names is never read, x included)
        assert bool(bad.any())
        for k, poison in (("actions", float("nan")), ("logp_old", float("inf")), ("advantages", float("nan")), ("returns", -float("inf"))):
            p[k] = p[k].clone()
            p[k][bad] = poison
    for u, v in zip(clean, run(dirty)):
        assert torch.equal(u, v)
    assert torch.isfinite(clean[2][:12]).all() and torch.isfinite(clean[0]).all()


# ---------------------------------------------------------------------------------------------- 5. determinism
def test_same_bits_on_every_stream_repetition_and_replay(eng):
    rows, bounds = STRIDE, [0, 6000, STRIDE]
    c = case(rows, 0, "quarter")
    actor, critic, log_std, _ = on_device(c)
    parts = shards_on_device(cut(c, bounds))
    shards = [(parts[0], None), (parts[1], index_list(bounds[2] - bounds[1], 9))]
    first = sharded_call(eng, actor, critic, log_std, shards, "tanh")[:3]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        second = sharded_call(eng, actor, critic, log_std, shards, "tanh")[:3]
    side.synchronize()
    third = sharded_call(eng, actor, critic, log_std, shards, "tanh")[:3]
    for other in (second, third):
        for u, v in zip(first, other):
            assert torch.equal(u, v)
    # the whole of ppo_grad_sharded, on one device, replayed from a captured graph
    rep = pyflyt_amd.Replicas(dict(actor=actor, critic=critic, log_std=log_std), [DEV, DEV])
    xs = [p["x"] for p in parts]
    batches = [(p["actions"], p["logp_old"], p["advantages"], p["returns"]) for p in parts]
    kw = dict(rows=[None, shards[1][1]], valid=[p["valid"] for p in parts], **COEF)
    eager = pyflyt_amd.ppo_grad_sharded([eng, eng], xs, rep, batches, **kw)
    flat = torch.cat([p.grad.reshape(-1) for p in params_of(actor, critic, log_std)[:-1]])
    assert torch.equal(flat, first[0]) and torch.equal(log_std.grad, first[1]) and torch.equal(eager, first[2])
    assert flat.data_ptr() != rep._grad.data_ptr() and actor[0].weight.grad.data_ptr() == rep._grad.data_ptr()  # (.grad: views of the one buffer)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stats = pyflyt_amd.ppo_grad_sharded([eng, eng], xs, rep, batches, **kw)
    for _ in range(2):
        rep._grad.fill_(float("nan"))
        log_std.grad.fill_(float("nan"))
        stats.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(rep._grad, first[0]) and torch.equal(log_std.grad, first[1]) and torch.equal(stats, first[2])


# ---------------------------------------------------------------------------------------------- 6. pf_moments_merge
def moments_of(x):
    """(count, mean[D], M2[D]) of the rows of x [n, D], in float64."""
    n = x.shape[0]
    if n == 0:
        return torch.zeros(1 + 2 * x.shape[1], dtype=torch.float64)
    mean = x.mean(0)
    return torch.cat([torch.tensor([float(n)], dtype=torch.float64), mean, ((x - mean) ** 2).sum(0)])


def chan(dst, blocks, D):
    n, mean, m2 = float(dst[0]), dst[1:1 + D].clone(), dst[1 + D:].clone()
    for b in blocks:
        nb = float(b[0])
        if nb == 0.0:
            continue
        d = b[1:1 + D] - mean
        tot = n + nb
        mean = mean + d * (nb / tot)
        m2 = m2 + b[1 + D:] + d * d * (n * nb / tot)
        n = tot
    return torch.cat([torch.tensor([n], dtype=torch.float64), mean, m2])


@pytest.mark.parametrize("D", [1, 21, 128])
@pytest.mark.parametrize("n_src", [1, 3, 16])
def test_moments_merge_against_chan_in_float64(eng, D, n_src):
    g = torch.Generator().manual_seed(1000 * D + n_src)
    sizes = [int(s) for s in torch.randint(1, 400, (n_src + 1,), generator=g)]
    if n_src > 1:
        sizes[2] = 0  # an empty block among them
    # (blocks as the shards of one env give them: columns of one scale and offset, the blocks' own means half a unit apart)
    scale, offset = 1.0 + 3.0 * torch.rand(D, generator=g, dtype=torch.float64), 5.0 * torch.randn(D, generator=g, dtype=torch.float64)
    data = [torch.randn(s, D, generator=g, dtype=torch.float64) * scale + offset + 0.5 * torch.randn(D, generator=g, dtype=torch.float64) for s in sizes]
    blocks = [moments_of(x) for x in data]
    dst = blocks[0].to(DEV)
    eng.moments_merge(dst, [b.to(DEV) for b in blocks[1:]])
    want = chan(blocks[0], blocks[1:], D)
    big = max(float(b.abs().max()) for b in blocks)
    err = float((dst.cpu() - want).abs().max())
    print(f"D {D} n_src {n_src}: max error {err:.3e}, {err / (2.0 ** -52 * big):.2f} ulps of the largest input {big:.3e}")
    assert err <= 64 * 2.0 ** -52 * big and float(dst[0]) == float(sum(sizes))
    direct = moments_of(torch.cat(data))  # (and the merged block describes the concatenated rows)
    assert float((dst.cpu() - direct).abs().max()) <= 1e-9 * big
    # into an empty dst: the block's own bits; empty blocks: nothing
    empty = torch.zeros(1 + 2 * D, dtype=torch.float64, device=DEV)
    eng.moments_merge(empty, [blocks[1].to(DEV)])
    assert torch.equal(empty.cpu(), blocks[1])
    before = dst.clone()
    eng.moments_merge(dst, [torch.zeros(1 + 2 * D, dtype=torch.float64, device=DEV)] * 2)
    assert torch.equal(dst, before)


# ---------------------------------------------------------------------------------------------- 7. the raw ABI's refusals
def _raises(fragment, fn):
    with pytest.raises(PyFlytAmdError) as e:
        fn()
    assert e.value.code == L.ERR_ARG and fragment in str(e.value), str(e.value)


def test_refusals_name_the_argument(eng):
    rows = 100
    c = case(rows, 0, "quarter")
    actor, critic, log_std, b = on_device(c)
    la, lc = layers_of(actor), layers_of(critic)
    A, SENT, lib, ctx = 4, -12345.0, eng.lib, eng._ctx
    f64 = dict(dtype=torch.float64, device=DEV)
    sums, block, stats = torch.full((4,), SENT, **f64), torch.full((24,), SENT, **f64), torch.full((16,), SENT, **f64)
    numel = eng.grad_numel([tuple(w.shape) for w, _ in la], [tuple(w.shape) for w, _ in lc])
    flat, out, gls = torch.full((numel,), SENT, device=DEV), torch.full((numel,), SENT, device=DEV), torch.full((A,), SENT, device=DEV)
    idx = torch.arange(rows, dtype=torch.int32, device=DEV)
    adv, valid, total = b["advantages"], b["valid"], torch.tensor([75.0, 1.0, 300.0, 0.0], **f64)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    run = lambda fn, *a: (lambda: L.check(fn(*a, eng._stream()), a[0]))  # noqa: E731

    who = "pf_ppo_adv_sums: "
    _raises(who + "m must be >= 1", run(lib.pf_ppo_adv_sums, ctx, p(adv), p(valid), None, 0, rows, p(sums)))
    _raises(who + "m must be below", run(lib.pf_ppo_adv_sums, ctx, p(adv), p(valid), None, (1 << 31) - 64, rows, p(sums)))
    _raises(who + "ctx is required", run(lib.pf_ppo_adv_sums, None, p(adv), p(valid), None, rows, rows, p(sums)))
    _raises(who + "advantages is required", run(lib.pf_ppo_adv_sums, ctx, None, p(valid), None, rows, rows, p(sums)))
    _raises(who + "sums is required", run(lib.pf_ppo_adv_sums, ctx, p(adv), p(valid), None, rows, rows, None))
    _raises(who + "rows_total must be >= 1", run(lib.pf_ppo_adv_sums, ctx, p(adv), p(valid), p(idx), rows, 0, p(sums)))
    _raises(who + "advantages and sums overlap", run(lib.pf_ppo_adv_sums, ctx, p(adv), p(valid), None, rows, rows, p(adv)))
    _raises(who + "row_index and sums overlap", run(lib.pf_ppo_adv_sums, ctx, p(adv), p(valid), p(idx), rows, rows, C.c_void_p(idx.data_ptr() + 8)))

    def src_array(ts):
        arr = (C.c_void_p * 16)()
        for g, t in enumerate(ts):
            arr[g] = None if t is None else t.data_ptr()
        return arr

    for fn, who, tail, words in ((lib.pf_adv_sums_add, "pf_adv_sums_add: ", (), 4), (lib.pf_moments_merge, "pf_moments_merge: ", (1,), 3)):
        dst, src = torch.full((words,), SENT, **f64), torch.ones(words, **f64)
        _raises(who + "n_src must be in 1..PF_PPO_MAX_SHARDS", run(fn, ctx, p(dst), src_array([src]), 0, *tail))
        _raises(who + "n_src must be in 1..PF_PPO_MAX_SHARDS", run(fn, ctx, p(dst), src_array([src]), 17, *tail))
        _raises(who + "ctx is required", run(fn, None, p(dst), src_array([src]), 1, *tail))
        _raises(who + "dst is required", run(fn, ctx, None, src_array([src]), 1, *tail))
        _raises(who + "src is required", run(fn, ctx, p(dst), None, 1, *tail))
        _raises(who + "src[1] is required", run(fn, ctx, p(dst), src_array([src, None]), 2, *tail))
        _raises(who + "src[1] and dst overlap", run(fn, ctx, p(dst), src_array([src, dst]), 2, *tail))
        torch.cuda.synchronize()
        assert bool((dst == SENT).all())
    _raises("pf_moments_merge: D must be in 1..128", run(lib.pf_moments_merge, ctx, p(sums), src_array([total]), 1, 0))
    _raises("pf_moments_merge: D must be in 1..128", run(lib.pf_moments_merge, ctx, p(sums), src_array([total]), 1, 129))

    # pf_ppo_grad_shard: what it adds to pf_ppo_grad_rows's refusals (those are test_gpu_ppo_grad_rows.py's: the checks are shared)
    qa, qc = eng._mlp_block(b["x"], la, "tanh")[0], eng._mlp_block(b["x"], lc, "tanh")[0]
    need = lib.pf_ppo_grad_workspace_bytes(C.byref(qa), C.byref(qc), rows)
    ws = torch.full((need // 8 + 1,), SENT, **f64)

    def shard(**kw):
        f = dict(ctx=ctx, m=rows, rows_total=rows, idx=idx, adv_sums=total, block=block, gls=None, stats=None, ws=ws, bytes=need, x=b["x"])
        f.update(kw)
        a = L.PfPpoGradArgs()
        a.clip, a.vf_coef, a.ent_coef, a.normalize_advantage = COEF["clip"], COEF["vf_coef"], COEF["ent_coef"], 1
        a.actor, a.critic = C.addressof(qa), C.addressof(qc)
        a.x, a.log_std, a.actions, a.logp_old = f["x"].data_ptr(), log_std.data_ptr(), b["actions"].data_ptr(), b["logp_old"].data_ptr()
        a.advantages, a.returns, a.valid = adv.data_ptr(), b["returns"].data_ptr(), valid.data_ptr()
        a.grad_log_std, a.stats = (None if f["gls"] is None else f["gls"].data_ptr()), (None if f["stats"] is None else f["stats"].data_ptr())
        eng._flat_grads([tuple(w.shape) for w, _ in la], [tuple(w.shape) for w, _ in lc], flat, a.actor_grad_w, a.actor_grad_b, a.critic_grad_w, a.critic_grad_b)
        return lambda keep=a: L.check(lib.pf_ppo_grad_shard(f["ctx"], C.byref(a), None, p(f["idx"]), f["m"], f["rows_total"], p(f["adv_sums"]), p(f["block"]),
                                                            p(f["ws"]), f["bytes"], eng._stream()), f["ctx"])

    who = "pf_ppo_grad_shard: "
    _raises(who + "m must be >= 1", shard(m=0))
    _raises(who + "rows_total must be >= 1", shard(rows_total=0))
    _raises(who + "ctx is required", shard(ctx=None))
    _raises(who + "grad_log_std must be NULL", shard(gls=gls))
    _raises(who + "stats must be NULL", shard(stats=stats))
    _raises(who + "adv_sums is required", shard(adv_sums=None))
    _raises(who + "shard_block is required", shard(block=None))
    _raises(who + "workspace_bytes", shard(bytes=need - 1))
    _raises(who + "advantages and shard_block overlap", shard(block=adv))
    _raises(who + "adv_sums and shard_block overlap", shard(block=total))
    _raises(who + "adv_sums and workspace overlap", shard(adv_sums=ws))
    _raises(who + "shard_block and actor_grad_w[0] overlap", shard(block=flat))

    def combine(**kw):
        f = dict(ctx=ctx, n_shards=2, width=A, numel=numel, vf_coef=0.5, ent_coef=0.0, vclip=0, bnd=0, bounds_coef=0.0, blocks=[block, block], grads=[flat, flat],
                 adv_sums=total, grad_out=out, log_std=log_std, grad_log_std=gls, stats=stats, args=True)
        f.update(kw)
        a = L.PfPpoShardCombine()
        for k in ("n_shards", "width", "numel", "vf_coef", "ent_coef", "vclip", "bnd", "bounds_coef"):
            setattr(a, k, f[k])
        a.blocks, a.grads = src_array(f["blocks"]), src_array(f["grads"])
        for k in ("adv_sums", "grad_out", "log_std", "grad_log_std", "stats"):
            setattr(a, k, None if f[k] is None else f[k].data_ptr())
        return lambda keep=a: L.check(lib.pf_ppo_shard_combine(f["ctx"], C.byref(a) if f["args"] else None, eng._stream()), f["ctx"])

    who = "pf_ppo_shard_combine: "
    _raises(who + "n_shards must be in 1..PF_PPO_MAX_SHARDS", combine(n_shards=0))
    _raises(who + "n_shards must be in 1..PF_PPO_MAX_SHARDS", combine(n_shards=17))
    _raises(who + "ctx is required", combine(ctx=None))
    _raises(who + "the argument block is required", combine(args=False))
    _raises(who + "numel must be >= 1", combine(numel=0))
    _raises(who + "width must be in 1..8", combine(width=9))
    _raises(who + "vf_coef must be finite and >= 0", combine(vf_coef=-1.0))
    _raises(who + "ent_coef must be finite and >= 0", combine(ent_coef=float("nan")))
    _raises(who + "bounds_coef must be finite and >= 0", combine(bounds_coef=float("inf")))
    _raises(who + "vclip and bnd must be 0 or 1", combine(vclip=2))
    _raises(who + "blocks[1] is required", combine(blocks=[block, None]))
    _raises(who + "grads[0] is required", combine(grads=[None, flat]))
    for name in ("adv_sums", "grad_out", "log_std", "grad_log_std", "stats"):
        _raises(who + f"{name} is required", combine(**{name: None}))
    _raises(who + "grads[0] and grad_out overlap", combine(grad_out=flat))
    _raises(who + "blocks[0] and stats overlap", combine(stats=block))
    _raises(who + "adv_sums and stats overlap", combine(stats=total))
    _raises(who + "log_std and grad_log_std overlap", combine(grad_log_std=log_std))
    torch.cuda.synchronize()
    for t in (sums, block, stats, flat, out, gls, ws):
        assert bool((t == SENT).all())  # no refused call wrote anything
    shard()()  # (the unedited calls run)
    combine(n_shards=1)()
    torch.cuda.synchronize()
    assert not bool((block == SENT).any()) and not bool((out == SENT).any()) and torch.equal(out, flat)
    with pytest.raises(ValueError, match="adv_sums must be a contiguous float64 tensor"):
        eng.ppo_grad_shard(b["x"], la, lc, log_std.detach(), b["actions"], b["logp_old"], adv, b["returns"], total.float())
    with pytest.raises(ValueError, match="flats must hold one flat gradient per block"):
        eng.ppo_shard_combine([block], total, [flat, flat], log_std.detach())

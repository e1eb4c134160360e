"""pf_adam_step on the device: Adam / AdamW with global-norm clipping against torch.optim.AdamW + clip_grad_norm_ in float64 at the
tensor sets where the chunking can go wrong; an unreached clip is no clip; alignment; determinism over streams and repetitions;
skip_nonfinite; the learning rate on the device; a whole epoch captured in one graph; through autograd; checkpoints to and from
torch.optim.Adam; refusals; the example."""
import copy
import ctypes as C
import math
import os
import subprocess
import sys

import pytest
import torch

import pyflyt_amd
from pyflyt_amd import build_params
from pyflyt_amd import _lib as L
from pyflyt_amd.engine import BatchEngine
from test_gpu_mlp import _raises, bound_ratio, make_layers
from test_gpu_ppo_loss import CLIP, HALF_LOG_2PI, SHIFTS, f32, hand_written_loss, inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX10 = [(64, 21), (64,), (64, 64), (64,), (4, 64), (4,), (64, 21), (64,), (1, 64), (1,), (4,)]  # actor 21-64-64-4, critic 21-64-1, log_std
SIZES_C = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]
SETS = {
    "a": (EX10, False),
    "b": ([(1,)], False),
    "c": ([(SIZES_C[i % len(SIZES_C)],) for i in range(32)], False),
    "d": ([((1 << 20) + 3,)], False),
    "e": (EX10, True),  # every tensor a slice base[1 : 1 + n]: no pointer is 16-byte aligned
}
STEPS = 20


@pytest.fixture(scope="module")
def eng():
    """A context WITHOUT an env task: the call uses a context for its device and its error string only."""
    e = BatchEngine(build_params("quadx", "none"), 64, device=DEV)
    yield e
    e.close()


def grid_cap(eng):
    """The most workgroups a call takes, from the workspace size: a double per workgroup and a fixed header."""
    size = eng.lib.pf_adam_workspace_bytes
    header = size(1) - 8
    return (size(1 << 30) - header) // 8


def numel(shape):
    return math.prod(shape)


def device_tensor(shape, unaligned):
    n = numel(shape)
    if not unaligned:
        t = torch.zeros(shape, device=DEV)
        assert t.data_ptr() % 16 == 0
        return t
    t = torch.zeros(n + 1, device=DEV)[1:1 + n].view(shape)
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


_DRAWS = {}


def draws(shapes, steps=STEPS, seed=0):
    """(p0, [grads of step 0, ...]) on the host in float32, drawn once per (shapes, steps, seed) and never changed; a tensor's
    gradients have a scale of their own, so that the norm is not one tensor's."""
    key = (tuple(shapes), steps, seed)
    if key not in _DRAWS:
        g = torch.Generator().manual_seed(100 + seed)
        p0 = [torch.randn(s, generator=g) * 0.5 for s in shapes]
        grads = [[torch.randn(s, generator=g) * (0.02 * (1 + i % 5)) for i, s in enumerate(shapes)] for _ in range(steps)]
        _DRAWS[key] = (p0, grads)
    return _DRAWS[key]


def norms64(grads):
    return [math.sqrt(sum(float(g.double().pow(2).sum()) for g in step)) for step in grads]


class Ours:
    """pyflyt_amd.Adam over fresh device copies of p0, fed through gradient tensors with stable addresses."""

    def __init__(self, eng, p0, unaligned=False, **hp):
        self.params = [device_tensor(p.shape, unaligned) for p in p0]
        self.grads = [device_tensor(p.shape, unaligned) for p in p0]
        for t, p in zip(self.params, p0):
            t.copy_(p)
        self.opt = pyflyt_amd.Adam(eng, self.params, **hp)
        if unaligned:  # (the moments as well: the class allocates aligned ones)
            self.opt.exp_avg = [device_tensor(p.shape, True) for p in p0]
            self.opt.exp_avg_sq = [device_tensor(p.shape, True) for p in p0]

    def step(self, grads):
        for t, g in zip(self.grads, grads):
            t.copy_(g)
        self.opt.step(grads=self.grads)
        return self.opt.state.clone()

    def result(self):
        return [t.clone() for t in self.params], [t.clone() for t in self.opt.exp_avg], [t.clone() for t in self.opt.exp_avg_sq], self.opt.state.clone()


def torch_run(p0, grads, dtype, lr, betas, eps, weight_decay, max_grad_norm, state_dict=None, start=None):
    """torch.optim.AdamW + clip_grad_norm_ on the host in `dtype`; returns (params, exp_avg, exp_avg_sq) as float64 and the optimiser."""
    ps = [torch.nn.Parameter((p if start is None else start[i]).detach().cpu().to(dtype).clone()) for i, p in enumerate(p0)]
    opt = torch.optim.AdamW(ps, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
    if state_dict is not None:
        opt.load_state_dict(state_dict)
    for step in grads:
        for p, g in zip(ps, step):
            p.grad = g.to(dtype).clone()
        if max_grad_norm is not None and math.isfinite(max_grad_norm):
            torch.nn.utils.clip_grad_norm_(ps, max_grad_norm)
        opt.step()
    return ([p.detach().double() for p in ps], [opt.state[p]["exp_avg"].double() for p in ps], [opt.state[p]["exp_avg_sq"].double() for p in ps]), opt


def assert_within_bound(got, ref, ref32, label):
    """each of param, exp_avg, exp_avg_sq, every tensor: err / max(e32, 2^-24 max|ref|) <= 8; returns the largest ratio per kind"""
    worst = {}
    for kind, gs, rs, fs in zip(("param", "exp_avg", "exp_avg_sq"), got, ref, ref32):
        worst[kind] = max(bound_ratio(g.cpu().reshape(-1), r.reshape(-1), f.reshape(-1)) for g, r, f in zip(gs, rs, fs))
    print(f"{label}: err / max(e32, 2^-24 max|ref|): " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 8.0, (label, k, v)
    return worst


# ---------------------------------------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize("name", list(SETS))
def test_against_float64(eng, name):
    shapes, unaligned = SETS[name]
    if name == "d":
        assert (numel(shapes[0]) + 1023) // 1024 > grid_cap(eng) > 1  # (more chunks than the grid has workgroups)
    p0, grads = draws(shapes)
    norms = norms64(grads)
    lr = 1e-2
    for weight_decay in (0.0, 0.01):
        for clip in ("active", "never"):
            max_grad_norm = f32(0.25 * min(norms)) if clip == "active" else f32(4.0 * max(norms))
            ours = Ours(eng, p0, unaligned, lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
            hp = dict(lr=ours.opt.lr, betas=ours.opt.betas, eps=ours.opt.eps, weight_decay=ours.opt.weight_decay, max_grad_norm=max_grad_norm)
            states = [ours.step(g) for g in grads]
            got = ours.result()
            ref, _ = torch_run(p0, grads, torch.float64, **hp)
            ref32, _ = torch_run(p0, grads, torch.float32, **hp)
            assert_within_bound(got[:3], ref, ref32, f"set {name} weight_decay {weight_decay} clip {clip}")
            for s, st in enumerate(torch.stack(states).cpu().tolist()):
                coef = min(1.0, max_grad_norm / (norms[s] + 1e-6))
                assert st[0] == s + 1 and abs(st[1] - norms[s]) <= 1e-12 * norms[s], (s, st, norms[s])
                assert abs(st[2] - coef) <= 1e-12 * coef and (st[2] < 1.0) == (clip == "active"), (s, st, coef)
                assert st[3] == ours.opt.lr and st[4:] == [0.0, 0.0, 0.0, 0.0]
            assert float(got[3][0]) == STEPS
            assert all(float((a.cpu().double() - b.double()).abs().max()) > 0 for a, b in zip(got[0], p0))  # (every tensor moved)


# ---------------------------------------------------------------------------------------------- 2. an unreached clip is no clip
def test_unreached_clip_is_no_clip(eng):
    p0, grads = draws(EX10, steps=5)
    far = f32(1e6 * max(norms64(grads)))
    a, b = Ours(eng, p0, max_grad_norm=None, weight_decay=0.01), Ours(eng, p0, max_grad_norm=far, weight_decay=0.01)
    for g in grads:
        sa, sb = a.step(g), b.step(g)
        assert float(sa[2]) == 1.0 and float(sb[2]) == 1.0 and torch.equal(sa, sb)
    for xs, ys in zip(a.result()[:3], b.result()[:3]):
        assert all(torch.equal(x, y) for x, y in zip(xs, ys))
    assert a.opt.stats_dict()["step"] == 5 and a.opt.stats_dict()["clip_coef"] == 1.0


# ---------------------------------------------------------------------------------------------- 3. alignment
def test_alignment_changes_no_bit(eng):
    p0, grads = draws(EX10, steps=5)
    hp = dict(lr=1e-2, weight_decay=0.01, max_grad_norm=f32(0.25 * min(norms64(grads))))
    a, b = Ours(eng, p0, False, **hp), Ours(eng, p0, True, **hp)
    for g in grads:
        assert torch.equal(a.step(g), b.step(g))
    for xs, ys in zip(a.result()[:3], b.result()[:3]):
        assert all(torch.equal(x, y) for x, y in zip(xs, ys))
    assert float(a.opt.state[2]) < 1.0


# ---------------------------------------------------------------------------------------------- 4. determinism
def test_same_bits_on_every_stream_and_repetition(eng):
    shapes = EX10 + [(300 * 1024 + 7,)]  # (and more chunks than workgroups)
    p0, grads = draws(shapes, steps=3)
    hp = dict(lr=1e-2, weight_decay=0.01, max_grad_norm=f32(0.25 * min(norms64(grads))))

    def run():
        o = Ours(eng, p0, **hp)
        for g in grads:
            o.step(g)
        assert all(torch.equal(t.cpu(), g) for t, g in zip(o.grads, grads[-1]))  # (a clipped step leaves grad[] bit for bit)
        return o.result()

    first = run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        second = run()
    side.synchronize()
    third = run()
    assert float(first[3][2]) < 1.0 and float(first[3][0]) == 3
    for xs, ys, zs in zip(first[:3], second[:3], third[:3]):
        assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(xs, ys, zs))
    assert torch.equal(first[3], second[3]) and torch.equal(first[3], third[3])


# ---------------------------------------------------------------------------------------------- 5. skip_nonfinite
def test_skip_nonfinite(eng):
    p0, grads = draws(EX10, steps=3)
    bad = [g.clone() for g in grads[1]]
    bad[2][17, 5] = float("inf")
    hp = dict(lr=1e-2, weight_decay=0.01, max_grad_norm=0.05)
    o = Ours(eng, p0, skip_nonfinite=True, **hp)
    o.step(grads[0])
    after1 = o.result()
    s2 = o.step(bad)
    after2 = o.result()
    for xs, ys in zip(after1[:3], after2[:3]):
        assert all(torch.equal(x, y) for x, y in zip(xs, ys))
    assert s2.tolist() == [1.0, float("inf"), 0.0, o.opt.lr, 1.0, 0.0, 0.0, 0.0]
    o.step(grads[2])
    clean = Ours(eng, p0, skip_nonfinite=True, **hp)  # (a run that never saw the bad gradient)
    clean.step(grads[0])
    clean.step(grads[2])
    for xs, ys in zip(o.result()[:3], clean.result()[:3]):
        assert all(torch.equal(x, y) for x, y in zip(xs, ys))
    assert o.opt.stats_dict()["step"] == 2 and o.opt.stats_dict()["skipped"] == 1 and clean.opt.stats_dict()["skipped"] == 0
    # without the flag the arithmetic runs as written: coef = 0.05 / inf = 0, and 0 * inf = NaN where the infinity sits
    n = Ours(eng, p0, skip_nonfinite=False, **hp)
    n.step(grads[0])
    s2 = n.step(bad)
    assert s2.tolist()[:3] == [2.0, float("inf"), 0.0] and float(s2[4]) == 0.0
    assert bool(torch.isnan(n.params[2][17, 5])) and bool(torch.isnan(n.opt.exp_avg[2][17, 5]))
    none = Ours(eng, p0, skip_nonfinite=False, lr=1e-2)  # (no clipping: coef = inf / inf, a NaN everywhere, as torch's clamp gives)
    none.step(bad)
    assert all(bool(torch.isnan(t).all()) for t in none.params)


# ---------------------------------------------------------------------------------------------- 6. the learning rate on the device
def test_device_learning_rate(eng):
    p0, grads = draws(EX10, steps=4)
    lrs = [f32(x) for x in (1e-2, 7e-3, 0.0, 3e-4)]
    lr_t = torch.zeros((), device=DEV)
    a, b = Ours(eng, p0, lr=lr_t, max_grad_norm=0.05), Ours(eng, p0, lr=lrs[0], max_grad_norm=0.05)
    for lr, g in zip(lrs, grads):
        lr_t.fill_(lr)
        b.opt.lr = lr
        assert torch.equal(a.step(g), b.step(g)) and float(a.opt.state[3]) == lr
    for xs, ys in zip(a.result()[:3], b.result()[:3]):
        assert all(torch.equal(x, y) for x, y in zip(xs, ys))


# ---------------------------------------------------------------------------------------------- 7. a whole epoch in one graph
def test_epoch_is_capturable(eng):
    M, A, D = 1000, 4, 21
    base = inputs(M, A)
    g = torch.Generator().manual_seed(8)
    obs = torch.randn(M, D, generator=g).to(DEV)
    actor, critic = make_layers(D, (64, 64), A, seed=21), make_layers(D, (64,), 1, seed=22)
    log_std = torch.linspace(-0.8, 0.2, A, device=DEV)
    params = [t for pair in actor for t in pair] + [t for pair in critic for t in pair] + [log_std]
    assert [tuple(p.shape) for p in params] == EX10
    mean0 = eng.mlp_forward(obs, actor, "tanh").clone()
    gi = torch.Generator().manual_seed(6)
    z = ((torch.rand(M, A, generator=gi, dtype=torch.float64) * 2.0 - 1.0) * 3.9).to(DEV)
    actions = (mean0.double() + z * log_std.double().exp()).float()
    zz = (actions.double() - mean0.double()) * (-log_std.double()).exp()
    logp = (-0.5 * zz * zz - log_std.double() - HALF_LOG_2PI).sum(-1)
    logp_old = (logp - torch.tensor(SHIFTS, dtype=torch.float64)[torch.randint(0, 5, (M,), generator=gi)].to(DEV)).float()
    lr_t = torch.zeros((), device=DEV)
    opt = pyflyt_amd.Adam(eng, params, lr=lr_t, max_grad_norm=0.5)

    def epoch():
        mean, value = eng.mlp_forward(obs, actor, "tanh"), eng.mlp_forward(obs, critic, "tanh")
        gm, gv, gls, _ = eng.ppo_loss(mean, log_std, value, actions, logp_old, base["advantages"], base["returns"], valid=base["valid"], clip=CLIP,
                                      vf_coef=0.5, ent_coef=0.0078125)
        ga, gc = eng.mlp_backward(obs, gm, actor, "tanh"), eng.mlp_backward(obs, gv, critic, "tanh")
        opt.step(grads=[t for pair in ga for t in pair] + [t for pair in gc for t in pair] + [gls])

    everything = params + opt.exp_avg + opt.exp_avg_sq + [opt.state]
    start = [t.clone() for t in everything]

    def restore():
        for t, s in zip(everything, start):
            t.copy_(s)

    lrs = [f32(x) for x in (3e-3, 2e-3, 1e-3)]
    for lr in lrs:  # the eager epochs: the warm-up, and what the replays must reproduce
        lr_t.fill_(lr)
        epoch()
    eager = [t.clone() for t in everything]
    assert float(opt.state[0]) == 3 and not torch.equal(eager[0], start[0])
    restore()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        before = torch.cuda.memory_allocated(DEV)
        epoch()
        assert torch.cuda.memory_allocated(DEV) == before
    restore()  # (capturing runs nothing; the restore is for the reader)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(DEV)
    for lr in lrs:
        lr_t.fill_(lr)
        graph.replay()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(DEV) == before
    for want, got in zip(eager, everything):
        assert torch.equal(want, got)


# ---------------------------------------------------------------------------------------------- 8. through autograd
def test_autograd_epochs_against_float64(eng):
    M, A, D, EPOCHS = 1000, 4, 21, 3
    vf_coef, ent_coef, max_norm = 0.5, 0.0078125, 0.5
    g = torch.Generator().manual_seed(5)
    obs = torch.randn(M, D, generator=g).to(DEV)
    nn = torch.nn
    torch.manual_seed(11)
    actor = nn.Sequential(nn.Linear(D, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, A)).to(DEV)
    critic = nn.Sequential(nn.Linear(D, 64), nn.Tanh(), nn.Linear(64, 1)).to(DEV)
    log_std = nn.Parameter(torch.linspace(-0.8, 0.2, A, device=DEV))
    with torch.no_grad():  # (test_autograd_under_ppo_loss's batch: ratios away from the clip bounds under THIS actor)
        mean = actor(obs)
        gi = torch.Generator().manual_seed(6)
        z = ((torch.rand(M, A, generator=gi, dtype=torch.float64) * 2.0 - 1.0) * 3.9).to(DEV)
        actions = (mean.double() + z * log_std.double().exp()).float()
        zz = (actions.double() - mean.double()) * (-log_std.double()).exp()
        logp = (-0.5 * zz * zz - log_std.double() - HALF_LOG_2PI).sum(-1)
        d = torch.tensor(SHIFTS, dtype=torch.float64)[torch.randint(0, 5, (M,), generator=gi)].to(DEV)
        base = inputs(M, A)
        x = dict(actions=actions, logp_old=(logp - d).float(), advantages=base["advantages"], returns=base["returns"], valid=base["valid"])
    nets = {torch.float32: (copy.deepcopy(actor), copy.deepcopy(critic), nn.Parameter(log_std.detach().clone())),
            torch.float64: (copy.deepcopy(actor).double(), copy.deepcopy(critic).double(), nn.Parameter(log_std.detach().double()))}
    unused = nn.Parameter(torch.full((5,), 0.25, device=DEV))  # (never in the loss: its .grad stays None)
    p_ours = list(actor.parameters()) + list(critic.parameters()) + [log_std]
    opt = pyflyt_amd.Adam(eng, p_ours + [unused], lr=1e-3, max_grad_norm=max_norm)
    for _ in range(EPOCHS):
        loss, _ = pyflyt_amd.ppo_loss(eng, pyflyt_amd.mlp(eng, obs, actor), log_std, pyflyt_amd.mlp(eng, obs, critic), x["actions"], x["logp_old"],
                                      x["advantages"], x["returns"], valid=x["valid"], clip=CLIP, vf_coef=vf_coef, ent_coef=ent_coef, normalize_advantage=True)
        opt.zero_grad()
        loss.backward()
        norm = math.sqrt(sum(float(p.grad.double().pow(2).sum()) for p in p_ours))
        opt.step()
        assert unused.grad is None and abs(float(opt.state[1]) - norm) <= 1e-12 * norm  # (the unused parameter is not in the norm)
    assert torch.equal(unused, torch.full((5,), 0.25, device=DEV)) and float(opt.exp_avg[-1].abs().max()) == 0.0 and opt.stats_dict()["step"] == EPOCHS
    final = {}
    for dtype, (a, c, ls) in nets.items():
        ps = list(a.parameters()) + list(c.parameters()) + [ls]
        ref = torch.optim.Adam(ps, lr=opt.lr, betas=opt.betas, eps=opt.eps)
        for _ in range(EPOCHS):
            ref.zero_grad()
            hand_written_loss(a, c, ls, obs, x, dtype, vf_coef, ent_coef).backward()
            torch.nn.utils.clip_grad_norm_(ps, max_norm)
            ref.step()
        final[dtype] = [p.detach().double() for p in ps]
    names = [f"actor.{n}" for n, _ in actor.named_parameters()] + [f"critic.{n}" for n, _ in critic.named_parameters()] + ["log_std"]
    ratios = {n: bound_ratio(p.detach().reshape(-1), r.reshape(-1), f.reshape(-1)) for n, p, r, f in zip(names, p_ours, final[torch.float64], final[torch.float32])}
    print(f"autograd, {EPOCHS} epochs: err / max(e32, 2^-24 max|ref|): " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 8.0 for v in ratios.values()), ratios


# ---------------------------------------------------------------------------------------------- 9. checkpoints
def test_checkpoints_move_to_torch_and_back(eng):
    p0, grads = draws(EX10, steps=4)
    hp = dict(lr=f32(1e-2), betas=(f32(0.9), f32(0.999)), eps=f32(1e-8), weight_decay=0.0, max_grad_norm=None)
    ref, _ = torch_run(p0, grads, torch.float64, **hp)
    ref32, _ = torch_run(p0, grads, torch.float32, **hp)
    # ours for three steps, torch.optim.Adam for the fourth
    ours = Ours(eng, p0, lr=hp["lr"])
    for g in grads[:3]:
        ours.step(g)
    sd = ours.opt.state_dict()
    assert all(float(s["step"]) == 3.0 for s in sd["state"].values()) and len(sd["state"]) == len(p0)
    ps = [torch.nn.Parameter(t.cpu().clone()) for t in ours.params]
    topt = torch.optim.Adam(ps, lr=1.0)
    topt.load_state_dict(sd)
    assert topt.param_groups[0]["lr"] == hp["lr"] and tuple(topt.param_groups[0]["betas"]) == hp["betas"]
    for p, g in zip(ps, grads[3]):
        p.grad = g.clone()
    topt.step()
    assert all(float(topt.state[p]["step"]) == 4.0 for p in ps)
    got = ([p.detach() for p in ps], [topt.state[p]["exp_avg"] for p in ps], [topt.state[p]["exp_avg_sq"] for p in ps])
    assert_within_bound(got, ref, ref32, "ours x 3, torch x 1")
    # torch for three steps, ours for the fourth
    (tp, _, _), topt = torch_run(p0, grads[:3], torch.float32, **hp)
    back = Ours(eng, [t.float() for t in tp], lr=123.0, betas=(0.5, 0.5))
    back.opt.load_state_dict(topt.state_dict())
    assert back.opt.stats_dict()["step"] == 3 and back.opt.lr == hp["lr"] and back.opt.betas == hp["betas"]
    back.step(grads[3])
    assert back.opt.stats_dict()["step"] == 4
    assert_within_bound(back.result()[:3], ref, ref32, "torch x 3, ours x 1")


# ---------------------------------------------------------------------------------------------- 10. arguments
def test_refusals_name_the_argument(eng):
    shapes = [(5, 3), (7,), (1030,)]
    n = [numel(s) for s in shapes]
    kinds = ("param", "grad", "exp_avg", "exp_avg_sq")
    tens = {k: [torch.zeros(2 * m, device=DEV) for m in n] for k in kinds}  # (twice the size: room to slide a pointer into a neighbour)
    state, lr_dev = torch.zeros(8, dtype=torch.float64, device=DEV), torch.full((1,), 1e-3, device=DEV)
    need = eng.lib.pf_adam_workspace_bytes(sum(n))
    assert need == 8 * (grid_cap(eng) + (eng.lib.pf_adam_workspace_bytes(1) - 8) // 8)
    ws = torch.zeros(need // 8 + 8, dtype=torch.float64, device=DEV)

    def call(edit=None, **kw):
        a = L.PfAdam()
        a.n_tensors, a.skip_nonfinite, a.lr, a.lr_dev, a.beta1, a.beta2, a.eps, a.weight_decay, a.max_grad_norm = 3, 0, 1e-3, None, 0.9, 0.999, 1e-8, 0.0, 1.0
        a.state = state.data_ptr()
        for i in range(3):
            a.numel[i] = n[i]
            for k in kinds:
                getattr(a, k)[i] = tens[k][i].data_ptr()
        if edit:
            edit(a)
        b = dict(ctx=eng._ctx, a=C.byref(a), ws=ws.data_ptr(), bytes=need)
        b.update(kw)
        return lambda: L.check(eng.lib.pf_adam_step(b["ctx"], b["a"], b["ws"], b["bytes"], eng._stream()), b["ctx"])

    def setter(name, value, index=None):
        def edit(a):
            if index is None:
                setattr(a, name, value)
            else:
                getattr(a, name)[index] = value
        return edit

    def both(*edits):
        def edit(a):
            for e in edits:
                e(a)
        return edit

    nan, inf = float("nan"), float("inf")
    _raises("pf_adam_step: ctx is required", call(ctx=None))
    _raises("pf_adam_step: the argument block is required", call(a=None))
    _raises("pf_adam_step: state is required", call(setter("state", None)))
    _raises("pf_adam_step: workspace is required", call(ws=None))
    _raises("pf_adam_step: param[0] is required", call(setter("param", None, 0)))
    _raises("pf_adam_step: grad[2] is required", call(setter("grad", None, 2)))
    _raises("pf_adam_step: exp_avg[1] is required", call(setter("exp_avg", None, 1)))
    _raises("pf_adam_step: exp_avg_sq[2] is required", call(setter("exp_avg_sq", None, 2)))
    _raises("pf_adam_step: n_tensors must be in 1..", call(setter("n_tensors", 0)))
    _raises("pf_adam_step: n_tensors must be in 1..", call(setter("n_tensors", 33)))
    _raises("pf_adam_step: numel[1] must be >= 1", call(setter("numel", 0, 1)))
    _raises("pf_adam_step: numel[2] must be >= 1", call(setter("numel", -4, 2)))
    _raises("pf_adam_step: numel: the total must be below 2^31", call(both(setter("numel", 1 << 30, 0), setter("numel", 1 << 30, 1))))
    for bad in (-1e-3, nan, inf):
        _raises("pf_adam_step: lr must be finite and >= 0", call(setter("lr", bad)))
    for bad in (1.0, -0.1, nan):
        _raises("pf_adam_step: beta1 must be in [0, 1)", call(setter("beta1", bad)))
        _raises("pf_adam_step: beta2 must be in [0, 1)", call(setter("beta2", bad)))
    for bad in (0.0, -1e-8, nan, inf):
        _raises("pf_adam_step: eps must be finite and > 0", call(setter("eps", bad)))
    for bad in (-0.01, nan, inf):
        _raises("pf_adam_step: weight_decay must be finite and >= 0", call(setter("weight_decay", bad)))
    for bad in (0.0, -1.0, nan):
        _raises("pf_adam_step: max_grad_norm must be > 0", call(setter("max_grad_norm", bad)))
    for bad in (2, -1):
        _raises("pf_adam_step: skip_nonfinite must be 0 or 1", call(setter("skip_nonfinite", bad)))
    _raises("pf_adam_step: workspace_bytes", call(bytes=need - 1))  # (refused by size: the buffer itself is large enough)
    _raises("pf_adam_step: workspace_bytes", call(bytes=0))
    _raises("pf_adam_step: param[0] and grad[0] overlap", call(setter("grad", tens["param"][0].data_ptr() + 4 * (n[0] - 1), 0)))
    _raises("pf_adam_step: exp_avg_sq[1] and exp_avg[2] overlap", call(setter("exp_avg_sq", tens["exp_avg"][2].data_ptr() + 400, 1)))
    _raises("pf_adam_step: param[1] and param[2] overlap", call(setter("param", tens["param"][2].data_ptr(), 1)))
    _raises("pf_adam_step: grad[1] and state overlap", call(setter("grad", state.data_ptr() + 60, 1)))
    _raises("pf_adam_step: exp_avg[0] and workspace overlap", call(setter("exp_avg", ws.data_ptr() + need - 4, 0)))
    _raises("pf_adam_step: state and workspace overlap", call(setter("state", ws.data_ptr() + need - 8)))
    _raises("pf_adam_step: param[2] and lr_dev overlap", call(setter("lr_dev", tens["param"][2].data_ptr() + 4 * (n[2] - 1))))
    _raises("pf_adam_step: state and lr_dev overlap", call(setter("lr_dev", state.data_ptr() + 8)))
    call()()  # (the unedited call runs; with lr_dev the lr argument is not looked at; +infinity is no clipping)
    call(both(setter("lr_dev", lr_dev.data_ptr()), setter("lr", -1.0), setter("max_grad_norm", inf)))()
    torch.cuda.synchronize()
    assert state.tolist() == [2.0, 0.0, 1.0, float(lr_dev), 0.0, 0.0, 0.0, 0.0]
    # the Python layer
    ok = [torch.zeros(3, 2, device=DEV), torch.zeros(5, device=DEV)]
    with pytest.raises(ValueError, match=r"params: 1\.\.32 tensors"):
        pyflyt_amd.Adam(eng, [torch.zeros(2, device=DEV) for _ in range(33)])
    with pytest.raises(ValueError, match=r"params\[1\] is the same tensor as params\[0\]"):
        pyflyt_amd.Adam(eng, [ok[0], ok[0]])
    with pytest.raises(ValueError, match=r"params\[1\] must be a contiguous float32"):
        pyflyt_amd.Adam(eng, [ok[0], torch.zeros(4, 3, device=DEV).T])
    with pytest.raises(ValueError, match=r"params\[0\] must be a contiguous float32"):
        pyflyt_amd.Adam(eng, [torch.zeros(4, dtype=torch.float64, device=DEV)])
    with pytest.raises(ValueError, match=r"params\[1\] must be a contiguous float32 tensor .* on cuda:0, got .* on cpu"):
        pyflyt_amd.Adam(eng, [ok[0], torch.zeros(5)])
    opt = pyflyt_amd.Adam(eng, ok)
    with pytest.raises(ValueError, match=r"grads\[1\] must be a contiguous float32 tensor of shape \(5,\)"):
        opt.step(grads=[torch.zeros(3, 2, device=DEV), torch.zeros(4, device=DEV)])
    with pytest.raises(ValueError, match=r"exp_avg\[0\] must be a contiguous float32 tensor of shape \(3, 2\)"):
        eng.adam_step(ok, [torch.zeros_like(t) for t in ok], [torch.zeros(2, 3, device=DEV), torch.zeros(5, device=DEV)], [torch.zeros_like(t) for t in ok], opt.state)
    assert float(opt.state[0]) == 0.0


# ---------------------------------------------------------------------------------------------- 11. the example
def test_example_11_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "11_ppo_on_device_optimizer.py"), "256", "2"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "iteration 1" in out.stdout and "grad_norm" in out.stdout and "clip_coef" in out.stdout

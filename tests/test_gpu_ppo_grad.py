"""pf_ppo_grad, BatchEngine.ppo_grad and pyflyt_amd.ppo_grad on the device.

1. Against the composed path of the same library (mlp -> ppo_loss -> backward()): every weight and bias gradient bit for bit; stats and
   grad_log_std, whose double sums are taken in another order, within the reordering bound of a double sum, M 2^-53 sum |term|, with
   sum |term| taken in float64 on the host from the per-row terms; the order-free slots exactly.
2. Against torch autograd in float64 on the CPU over double copies of the networks, with test_gpu_mlp.py's tolerance for
   pf_mlp_backward: err <= 8 max(e32, 2^-24 max |ref|), e32 the error of torch's own float32 evaluation of the same loss.
3. Invalid rows: what they hold changes no bit; no valid row at all.   4. Determinism, capture, alignment.   5. The refusals of the
raw ABI.   6. What is left in .grad.   7. The example.

Shapes: rows 1, 63 / 64 / 65 (the ragged tile) and 64 * 256 + 1 (one workgroup strides to a second, ragged tile); the networks of NETS
(a second input chunk of one column, odd widths, two and three layers, widths of 1, the widest head, both critics). The batch is test_gpu_ppo_loss.py's, made under the float64 actor: |z| < 4, ratios at 0.67, 0.905, 1, 1.105, 1.49 with
clip = 0.2, so no branch of the objective is decided by rounding. ReLU against float64 only at the small row counts, for
test_gpu_mlp.py's reason (a hidden unit within rounding of 0 takes the other side of the derivative's jump in float32)."""
import copy
import ctypes as C
import math
import os
import subprocess
import sys

import pytest
import torch

import pyflyt_amd
from pyflyt_amd import PyFlytAmdError, build_params
from pyflyt_amd import _lib as L
from pyflyt_amd.engine import BatchEngine
from test_gpu_ppo_loss import CLIP, HALF_LOG_2PI, SHIFTS, f32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 2.0 ** -53
STRIDE = 64 * 256 + 1
#        D    actor's hidden  A  activation  critic's hidden
NETS = [(21, (64, 64), 4, "tanh", (64,)),
        (65, (64, 33), 7, "relu", (33, 64)),
        (123, (33,), 6, "tanh", (64,)),
        (1, (1,), 1, "relu", (33, 64)),
        (21, (64, 64), 8, "tanh", (33, 64))]
COEF = dict(clip=CLIP, vf_coef=0.5, ent_coef=0.0078125, normalize_advantage=True)  # (exact in float32)


@pytest.fixture(scope="module")
def eng():
    e = BatchEngine(build_params("quadx", "none"), 64, device=DEV)  # (a context WITHOUT an env task: any context serves)
    yield e
    e.close()


def sequential(sizes, activation):
    nn, mods = torch.nn, []
    for i, (a, b) in enumerate(zip(sizes[:-1], sizes[1:])):
        mods.append(nn.Linear(a, b))
        if i + 2 < len(sizes):
            mods.append(nn.Tanh() if activation == "tanh" else nn.ReLU())
    return nn.Sequential(*mods)


_CASES = {}


def case(rows, net, valid="quarter"):
    """The networks (float32, on the CPU: the tests copy them), log_std and the batch of one (rows, network, valid) case: made once,
    never changed."""
    key = (rows, net, valid)
    if key in _CASES:
        return _CASES[key]
    D, hidden, A, activation, chidden = NETS[net]
    torch.manual_seed(100 * net + 7)
    actor, critic = sequential([D, *hidden, A], activation), sequential([D, *chidden, 1], activation)
    g = torch.Generator().manual_seed(rows + 31 * net)
    log_std = (torch.rand(A, generator=g, dtype=torch.float64) * 1.5 - 1.0).float()
    x = torch.randn(rows, D, generator=g)
    with torch.no_grad():
        mean = copy.deepcopy(actor).double()(x.double())
        z = (torch.rand(rows, A, generator=g, dtype=torch.float64) * 2.0 - 1.0) * 3.9
        actions = (mean + z * log_std.double().exp()).float()
        zz = (actions.double() - mean) * (-log_std.double()).exp()
        logp = (-0.5 * zz * zz - log_std.double() - HALF_LOG_2PI).sum(-1)
        d = torch.tensor(SHIFTS, dtype=torch.float64)[torch.randint(0, 5, (rows,), generator=g)]
    advantages = (torch.randn(rows, generator=g, dtype=torch.float64) * 2.0 + 0.3).float()
    returns = (torch.randn(rows, generator=g, dtype=torch.float64) * 3.0 + 1.0).float()
    if valid == "quarter":
        v = torch.rand(rows, generator=g) >= 0.25
        v[0] = True
    else:
        v = None if valid is None else torch.zeros(rows, dtype=torch.bool)
    c = dict(actor=actor, critic=critic, log_std=log_std, x=x, actions=actions, logp_old=(logp - d).float(), advantages=advantages, returns=returns,
             valid=v, activation=activation)
    _CASES[key] = c
    return c


def on_device(c):
    """(actor, critic, log_std as a Parameter, the batch's tensors) as fresh device copies."""
    actor, critic = copy.deepcopy(c["actor"]).to(DEV), copy.deepcopy(c["critic"]).to(DEV)
    log_std = torch.nn.Parameter(c["log_std"].to(DEV))
    b = {k: (None if c[k] is None else c[k].to(DEV).contiguous()) for k in ("x", "actions", "logp_old", "advantages", "returns", "valid")}
    return actor, critic, log_std, b


def params_of(actor, critic, log_std):
    return list(actor.parameters()) + list(critic.parameters()) + [log_std]


def composed(eng, actor, critic, log_std, b, coef=COEF):
    """The path this call replaces: returns ([gradients of the networks' parameters], grad_log_std, stats, mean, value)."""
    ps = params_of(actor, critic, log_std)
    for p in ps:
        p.grad = None
    mean, value = pyflyt_amd.mlp(eng, b["x"], actor), pyflyt_amd.mlp(eng, b["x"], critic)
    loss, stats = pyflyt_amd.ppo_loss(eng, mean, log_std, value, b["actions"], b["logp_old"], b["advantages"], b["returns"], valid=b["valid"], **coef)
    loss.backward()
    grads = [p.grad.clone() for p in ps]
    for p in ps:
        p.grad = None
    return grads[:-1], grads[-1], stats.clone(), mean.detach(), value.detach()


def layers_of(net):
    return [(m.weight.detach(), m.bias.detach()) for m in net if isinstance(m, torch.nn.Linear)]


def fused(eng, actor, critic, log_std, b, activation, coef=COEF):
    """([gradients of the networks' parameters], grad_log_std, stats) of BatchEngine.ppo_grad, as copies."""
    ga, gc, gls, stats = eng.ppo_grad(b["x"], layers_of(actor), layers_of(critic), log_std.detach(), b["actions"], b["logp_old"], b["advantages"],
                                      b["returns"], valid=b["valid"], actor_activation=activation, critic_activation=activation, **coef)
    return [t.clone() for net in (ga, gc) for pair in net for t in pair], gls.clone(), stats.clone()


def reorder_bounds(b, log_std, mean, value, stats, coef):
    """The largest admissible |fused - composed| of stats [16] and grad_log_std [A] when both sum the same per-row terms in double in
    another order: a raw sum S of M terms may move by M 2^-53 sum |t|. The terms, in float64 on the host from the composed path's
    means and values; the derived slots by first-order propagation through pf_ppo_loss's finish (w = 1 / c):
      policy_loss = -w S0; value_loss = w S1 / 2; loss = policy_loss + vf_coef value_loss - ent_coef H; approx_kl = w S2;
      explained variance = 1 - var_d / var_r, var_r = w S5 - (w S4)^2, var_d = w S1 - (w S6)^2.
    On top of each, 8 ulps (double) of the largest magnitude its few final operations see."""
    M, A = mean.shape
    v = torch.ones(M, dtype=torch.bool, device=DEV) if b["valid"] is None else b["valid"].bool()
    c = float(v.sum())
    w = 1.0 / c if c else 0.0
    ls = log_std.detach().double()
    a64 = b["advantages"].double()
    adv = a64
    if coef["normalize_advantage"]:
        adv = (a64 - float(stats[7])) / max(float(stats[8]), 1e-8)
    z = (b["actions"].double() - mean.double()) * torch.exp(-ls)
    d = (-0.5 * z * z - ls - HALF_LOG_2PI).sum(-1) - b["logp_old"].double()
    r = torch.exp(d)
    u, vv = r * adv, torch.clamp(r, 1.0 - coef["clip"], 1.0 + coef["clip"]) * adv
    live = v & (u <= vv)
    gl = torch.where(live, -w * adv * r, 0.0)
    ret, dv = b["returns"].double(), value.double().reshape(-1) - b["returns"].double()
    sabs = lambda t: float(torch.where(v, t.abs(), 0.0).sum())  # noqa: E731
    k = M * U64
    B0, B1, B2, B4, B5, B6 = (k * sabs(t) for t in (torch.minimum(u, vv), dv * dv, (r - 1.0) - d, ret, ret * ret, dv))
    sums = lambda t: float(torch.where(v, t, 0.0).sum())  # noqa: E731
    m_r, m_d = w * sums(ret), w * sums(dv)
    var_r, var_d = w * sums(ret * ret) - m_r * m_r, w * sums(dv * dv) - m_d * m_d
    e_vr, e_vd = w * B5 + 2.0 * abs(m_r) * w * B4, w * B1 + 2.0 * abs(m_d) * w * B6
    ulp = lambda *xs: 8.0 * U64 * max(abs(t) for t in xs)  # noqa: E731
    H = abs(float(stats[4]))
    bound = [0.0] * 16
    bound[2] = w * B0 + ulp(w * sabs(torch.minimum(u, vv)))
    bound[3] = 0.5 * w * B1 + ulp(w * sabs(dv * dv))
    bound[1] = bound[2] + coef["vf_coef"] * bound[3] + ulp(w * sabs(torch.minimum(u, vv)), w * sabs(dv * dv), coef["ent_coef"] * H)
    bound[5] = w * B2 + ulp(w * sabs((r - 1.0) - d))
    if c and var_r > 0.0:
        e_vr, e_vd = e_vr + ulp(w * sabs(ret * ret)), e_vd + ulp(w * sabs(dv * dv))
        bound[9] = e_vd / var_r + abs(var_d) * e_vr / (var_r * var_r) + ulp(1.0, var_d / var_r)
    t_gls = gl.unsqueeze(-1) * (z * z - 1.0)
    gb = [k * float(t_gls[:, cix].abs().sum()) for cix in range(A)]
    return bound, gb


def check_against_composed(eng, rows, net, valid, coef=COEF):
    c = case(rows, net, valid)
    actor, critic, log_std, b = on_device(c)
    want, want_gls, want_stats, mean, value = composed(eng, actor, critic, log_std, b, coef)
    got, got_gls, got_stats = fused(eng, actor, critic, log_std, b, c["activation"], coef)
    names = [f"actor.{n}" for n, _ in actor.named_parameters()] + [f"critic.{n}" for n, _ in critic.named_parameters()]
    for name, g, w in zip(names, got, want):
        assert g.shape == w.shape and torch.isfinite(g).all(), name
        assert torch.equal(g, w), (name, float((g - w).abs().max()))
    n_actor = len(list(actor.parameters()))
    # (the output biases: a lone ReLU unit may be dead. One row alone has the normalised advantage 0, or may sit on the clipped branch)
    assert float(got[-1].abs().max()) > 0 and (rows == 1 or float(got[n_actor - 1].abs().max()) > 0)
    bound, gb = reorder_bounds(b, log_std, mean, value, want_stats, coef)
    gs, ws = got_stats.tolist(), want_stats.tolist()
    line = []
    for slot in (0, 4, 6, 7, 8, 10, 11, 12, 13, 14, 15):  # the count, H, the clip fraction (a sum of whole numbers), mu, sigma, min r, max r
        assert gs[slot] == ws[slot] or (math.isnan(gs[slot]) and math.isnan(ws[slot])), (slot, gs[slot], ws[slot])
    for slot in (1, 2, 3, 5, 9):
        if math.isnan(ws[slot]):
            assert math.isnan(gs[slot]), (slot, gs[slot])
            continue
        line.append(f"stats[{slot}] {abs(gs[slot] - ws[slot]):.2e} <= {bound[slot]:.2e}")
        assert abs(gs[slot] - ws[slot]) <= bound[slot], (slot, gs[slot], ws[slot], bound[slot])
    for cix, (g, w) in enumerate(zip(got_gls.tolist(), want_gls.tolist())):
        lim = gb[cix] + 2.0 ** -23 * abs(w) * 1.0  # (one float32 ulp of the result, at most 2^-23 |result|)
        line.append(f"gls[{cix}] {abs(g - w):.2e} <= {lim:.2e}")
        assert abs(g - w) <= lim, (cix, g, w, lim)
    print(f"rows {rows} net {NETS[net]} valid {valid}: " + ", ".join(line))


# ---------------------------------------------------------------------------------------------- 1. the composed path
@pytest.mark.parametrize("rows", [1, 63, 64, 65, STRIDE])
@pytest.mark.parametrize("net", range(len(NETS)))
def test_bits_of_the_composed_path(eng, rows, net):
    check_against_composed(eng, rows, net, "quarter")
    if rows == 1:  # (sigma = 0 makes the one normalised advantage 0: the raw advantage as well)
        check_against_composed(eng, rows, net, "quarter", dict(COEF, normalize_advantage=False))


@pytest.mark.parametrize("rows, net, valid", [(65, 0, None), (STRIDE, 0, None), (STRIDE, 2, None), (64, 1, None)])
def test_bits_of_the_composed_path_without_valid(eng, rows, net, valid):
    check_against_composed(eng, rows, net, valid)


def test_bits_without_normalisation_and_with_other_coefficients(eng):
    check_against_composed(eng, 65, 0, "quarter", dict(clip=0.1, vf_coef=2.0, ent_coef=0.0, normalize_advantage=False))
    check_against_composed(eng, STRIDE, 4, "quarter", dict(clip=0.3, vf_coef=1.0, ent_coef=0.25, normalize_advantage=False))


# ---------------------------------------------------------------------------------------------- 2. float64 on the CPU
def written_out_loss(actor, critic, log_std, c, dtype, coef):
    """test_gpu_ppo_loss.py's reference(), written out over the networks: the contract in `dtype` on the float32 inputs; mu and sigma in
    float64 and handed to the rows as their float32 roundings."""
    clip, vf_coef, ent_coef = f32(coef["clip"]), f32(coef["vf_coef"]), f32(coef["ent_coef"])
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
    policy_loss = -(torch.where(v, surr, zero).sum() * wt)
    value_loss = 0.5 * (torch.where(v, (value - c["returns"].to(dtype)) ** 2, zero).sum() * wt)
    return policy_loss + vf_coef * value_loss - ent_coef * (log_std + (0.5 + HALF_LOG_2PI)).sum()


def cpu_gradients(c, dtype, coef):
    actor, critic = copy.deepcopy(c["actor"]).to(dtype), copy.deepcopy(c["critic"]).to(dtype)
    log_std = torch.nn.Parameter(c["log_std"].to(dtype))
    written_out_loss(actor, critic, log_std, c, dtype, coef).backward()
    return [p.grad.double() for p in params_of(actor, critic, log_std)]


F64_CASES = [(1, 0, "quarter"), (63, 1, "quarter"), (64, 3, "quarter"), (65, 1, "quarter"), (65, 2, None), (65, 4, "quarter"),
             (STRIDE, 0, "quarter"), (STRIDE, 2, "quarter"), (STRIDE, 4, None)]


@pytest.mark.parametrize("rows, net, valid", F64_CASES)
def test_against_float64_autograd(eng, rows, net, valid):
    c = case(rows, net, valid)
    g64, g32 = cpu_gradients(c, torch.float64, COEF), cpu_gradients(c, torch.float32, COEF)
    actor, critic, log_std, b = on_device(c)
    got, got_gls, _ = fused(eng, actor, critic, log_std, b, c["activation"])
    names = [f"actor.{n}" for n, _ in actor.named_parameters()] + [f"critic.{n}" for n, _ in critic.named_parameters()] + ["log_std"]
    ratios = {}
    for name, g, ref, e32 in zip(names, got + [got_gls], g64, g32):
        err = float((g.double().cpu() - ref).abs().max())
        ratios[name] = err / max(float((e32 - ref).abs().max()), 2.0 ** -24 * float(ref.abs().max()), 1e-300)
    print(f"rows {rows} net {NETS[net]} valid {valid}: err / max(e32, 2^-24 max|ref|): " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    for k, v in ratios.items():
        assert v <= 8.0, (k, v)


# ---------------------------------------------------------------------------------------------- 3. invalid rows
@pytest.mark.parametrize("rows, net", [(65, 0), (STRIDE, 1)])
def test_invalid_rows_reach_no_output(eng, rows, net):
    c = case(rows, net, "quarter")
    actor, critic, log_std, b = on_device(c)
    clean = fused(eng, actor, critic, log_std, b, c["activation"])
    bad = ~b["valid"]
    assert abs(int(bad.sum()) - rows // 4) <= max(8, rows // 50)
    p = dict(b)
    for k, poison in (("actions", float("nan")), ("logp_old", float("inf")), ("advantages", float("nan")), ("returns", -float("inf"))):
        p[k] = b[k].clone()
        p[k][bad] = poison
    dirty = fused(eng, actor, critic, log_std, p, c["activation"])
    for u, v in zip(clean[0] + [clean[1], clean[2]], dirty[0] + [dirty[1], dirty[2]]):
        assert torch.equal(u, v)  # (slot 9 is finite here: a NaN would compare unequal)
    assert torch.isfinite(clean[2][:12]).all()


@pytest.mark.parametrize("rows, net", [(65, 0), (STRIDE, 4)])
def test_no_valid_row(eng, rows, net):
    c = case(rows, net, "none")
    actor, critic, log_std, b = on_device(c)
    grads, gls, stats = fused(eng, actor, critic, log_std, b, c["activation"])
    for g in grads:
        assert torch.equal(g, torch.zeros_like(g))
    assert torch.equal(gls, torch.full_like(gls, -COEF["ent_coef"]))
    s = stats.tolist()
    H = float((log_std.detach().double() + (0.5 + HALF_LOG_2PI)).sum())
    assert s[0] == 0.0 and s[2] == 0.0 and s[3] == 0.0 and s[5:9] == [0.0] * 4 and math.isnan(s[9])
    assert s[10] == float("inf") and s[11] == -float("inf") and s[12:] == [0.0] * 4
    assert abs(s[4] - H) <= 8 * U64 * abs(H) and s[1] == 0.0 - COEF["ent_coef"] * s[4]
    _, want_gls, want_stats, _, _ = composed(eng, actor, critic, log_std, b)  # (pf_ppo_loss's c = 0 clause, slot by slot)
    assert torch.equal(gls, want_gls)
    assert all(x == y or (math.isnan(x) and math.isnan(y)) for x, y in zip(s, want_stats.tolist()))


# ---------------------------------------------------------------------------------------------- 4. determinism, capture, alignment
def test_same_bits_on_every_stream_repetition_and_replay(eng):
    c = case(STRIDE, 0, "quarter")
    actor, critic, log_std, b = on_device(c)
    first = fused(eng, actor, critic, log_std, b, "tanh")
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        second = fused(eng, actor, critic, log_std, b, "tanh")
    side.synchronize()
    third = fused(eng, actor, critic, log_std, b, "tanh")
    args = (b["x"], layers_of(actor), layers_of(critic), log_std.detach(), b["actions"], b["logp_old"], b["advantages"], b["returns"])
    kw = dict(valid=b["valid"], actor_activation="tanh", critic_activation="tanh", **COEF)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        before = torch.cuda.memory_allocated(DEV)
        ga, gc, gls, stats = eng.ppo_grad(*args, **kw)
        assert torch.cuda.memory_allocated(DEV) == before  # (no allocation: the engine's tensors of this shape exist)
    outs = [t for net in (ga, gc) for pair in net for t in pair] + [gls, stats]
    for _ in range(2):
        for t in outs:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for want, got in zip(first[0] + [first[1], first[2]], outs):
            assert torch.equal(want, got)
    for other in (second, third):
        for u, v in zip(first[0] + [first[1], first[2]], other[0] + [other[1], other[2]]):
            assert torch.equal(u, v)


def test_unaligned_rows_give_the_same_bits(eng):
    """The four-wide rows (actions) and every other operand one float past a 16-byte boundary."""
    c = case(STRIDE, 0, "quarter")
    actor, critic, log_std, b = on_device(c)
    aligned = fused(eng, actor, critic, log_std, b, "tanh")
    shifted = dict(b)
    for k in ("x", "actions", "logp_old", "advantages", "returns"):
        buf = torch.empty(b[k].numel() + 1, device=DEV)
        view = buf[1:].view(b[k].shape)
        view.copy_(b[k])
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        shifted[k] = view
    off = fused(eng, actor, critic, log_std, shifted, "tanh")
    for u, v in zip(aligned[0] + [aligned[1], aligned[2]], off[0] + [off[1], off[2]]):
        assert torch.equal(u, v)


# ---------------------------------------------------------------------------------------------- 5. the raw ABI's refusals
def _raises(fragment, fn):
    with pytest.raises(PyFlytAmdError) as e:
        fn()
    assert e.value.code == L.ERR_ARG and fragment in str(e.value), str(e.value)


def test_refusals_name_the_argument(eng):
    rows, D, A = 100, 21, 4
    c = case(rows, 0, "quarter")
    actor, critic, log_std, b = on_device(c)
    la, lc = layers_of(actor), layers_of(critic)
    x2 = torch.zeros(2 * rows, D, device=DEV)  # (room behind x for the overlapping pointers)
    x2[:rows] = b["x"]
    SENT = -12345.0
    outs = dict(aw=[torch.full_like(w, SENT) for w, _ in la], ab=[torch.full_like(v, SENT) for _, v in la],
                cw=[torch.full_like(w, SENT) for w, _ in lc], cb=[torch.full_like(v, SENT) for _, v in lc],
                gls=torch.full((A,), SENT, device=DEV), stats=torch.full((16,), SENT, dtype=torch.float64, device=DEV))
    q0a, q0c = eng._mlp_block(x2[:rows], la, "tanh")[0], eng._mlp_block(x2[:rows], lc, "tanh")[0]
    need = eng.lib.pf_ppo_grad_workspace_bytes(C.byref(q0a), C.byref(q0c), rows)
    Pa, Pc = (sum(w.numel() + v.numel() for w, v in ls) for ls in (la, lc))
    assert need == 2 * (4 * (Pa + Pc) + 8 * 20)  # two workgroups: a block of float partials per network and a row of twenty doubles
    ws = torch.full((need // 8 + 1,), SENT, dtype=torch.float64, device=DEV)

    def call(edit=None, **kw):
        qa, qc = eng._mlp_block(x2[:rows], la, "tanh")[0], eng._mlp_block(x2[:rows], lc, "tanh")[0]
        if edit:
            edit(qa, qc)
        f = dict(ctx=eng._ctx, actor=C.addressof(qa), critic=C.addressof(qc), x=x2.data_ptr(), log_std=log_std.data_ptr(), actions=b["actions"].data_ptr(),
                 logp_old=b["logp_old"].data_ptr(), advantages=b["advantages"].data_ptr(), returns=b["returns"].data_ptr(), valid=b["valid"].data_ptr(),
                 grad_log_std=outs["gls"].data_ptr(), stats=outs["stats"].data_ptr(), rows=rows, ws=ws.data_ptr(), bytes=need, args=True,
                 aw=[t.data_ptr() for t in outs["aw"]], ab=[t.data_ptr() for t in outs["ab"]], cw=[t.data_ptr() for t in outs["cw"]],
                 cb=[t.data_ptr() for t in outs["cb"]], **COEF)
        f.update(kw)
        a = L.PfPpoGradArgs()
        a.clip, a.vf_coef, a.ent_coef, a.normalize_advantage = f["clip"], f["vf_coef"], f["ent_coef"], int(f["normalize_advantage"])
        for name in ("actor", "critic", "x", "log_std", "actions", "logp_old", "advantages", "returns", "valid", "grad_log_std", "stats"):
            setattr(a, name, f[name])
        for field, key in (("actor_grad_w", "aw"), ("actor_grad_b", "ab"), ("critic_grad_w", "cw"), ("critic_grad_b", "cb")):
            for l, p in enumerate(f[key]):
                getattr(a, field)[l] = p

        def run(keep=(qa, qc, a)):
            L.check(eng.lib.pf_ppo_grad(f["ctx"], C.byref(a) if f["args"] else None, f["rows"], f["ws"], f["bytes"], eng._stream()), f["ctx"])
        return run

    def net_edit(which, name, value, index=None):
        def edit(qa, qc):
            q = qa if which == "actor" else qc
            if index is None:
                setattr(q, name, value)
            else:
                getattr(q, name)[index] = value
        return edit

    who = "pf_ppo_grad: "
    _raises(who + "ctx is required", call(ctx=None))
    _raises(who + "the argument block is required", call(args=False))
    for name in ("actor", "critic", "x", "log_std", "actions", "logp_old", "advantages", "returns", "grad_log_std", "stats"):
        _raises(who + f"{name} is required", call(**{name: None}))
    _raises(who + "workspace is required", call(ws=None))
    _raises(who + "actor_grad_w[1] is required", call(aw=[outs["aw"][0].data_ptr(), None, outs["aw"][2].data_ptr()]))
    _raises(who + "actor_grad_b[2] is required", call(ab=[outs["ab"][0].data_ptr(), outs["ab"][1].data_ptr(), None]))
    _raises(who + "critic_grad_w[0] is required", call(cw=[None, outs["cw"][1].data_ptr()]))
    _raises(who + "critic_grad_b[1] is required", call(cb=[outs["cb"][0].data_ptr(), None]))
    _raises(who + "rows must be >= 1", call(rows=0))
    _raises(who + "rows must be >= 1", call(rows=-3))
    _raises(who + "rows must be below", call(rows=(1 << 31) - 64))
    for net in ("actor", "critic"):
        _raises(who + f"{net}: n_layers must be 2 or 3", call(net_edit(net, "n_layers", 4)))
        _raises(who + f"{net}: width", call(net_edit(net, "width", 65, 0)))
        _raises(who + f"{net}: width", call(net_edit(net, "width", 0, 0)))
        _raises(who + f"{net}: in_dim must be in 1..128", call(net_edit(net, "in_dim", 129)))
        _raises(who + f"{net}: activation must be", call(net_edit(net, "activation", 2)))
        _raises(who + f"{net}: w / b", call(net_edit(net, "w", None, 1)))
        _raises(who + f"{net}: w / b", call(net_edit(net, "b", None, 0)))
    _raises(who + "actor: out_dim must be in 1..8", call(net_edit("actor", "out_dim", 9)))
    _raises(who + "critic: out_dim must be 1", call(net_edit("critic", "out_dim", 2)))
    _raises(who + "critic: in_dim must equal", call(net_edit("critic", "in_dim", D + 1)))
    _raises(who + "clip must be finite and > 0", call(clip=0.0))
    _raises(who + "clip must be finite and > 0", call(clip=float("inf")))
    _raises(who + "vf_coef must be finite and >= 0", call(vf_coef=-1.0))
    _raises(who + "ent_coef must be finite and >= 0", call(ent_coef=float("nan")))
    _raises(who + "normalize_advantage must be 0 or 1", call(normalize_advantage=2))
    _raises(who + "workspace_bytes", call(bytes=need - 1))  # (refused by size: the buffer itself is large enough)
    _raises(who + "workspace_bytes", call(bytes=0))
    _raises(who + "workspace must be 8-byte aligned", call(ws=ws.data_ptr() + 4))
    _raises(who + "x and workspace overlap", call(ws=x2.data_ptr() + 4 * D * rows - 8))
    _raises(who + "actions and stats overlap", call(stats=b["actions"].data_ptr()))
    _raises(who + "x and actor_grad_w[0] overlap", call(aw=[x2.data_ptr() + 4 * D, outs["aw"][1].data_ptr(), outs["aw"][2].data_ptr()]))
    _raises(who + "workspace and critic_grad_b[1] overlap", call(cb=[outs["cb"][0].data_ptr(), ws.data_ptr() + need - 4]))
    _raises(who + "grad_log_std and actor_grad_b[2] overlap", call(ab=[outs["ab"][0].data_ptr(), outs["ab"][1].data_ptr(), outs["gls"].data_ptr()]))
    _raises(who + "returns and grad_log_std overlap", call(grad_log_std=b["returns"].data_ptr()))
    torch.cuda.synchronize()
    every = outs["aw"] + outs["ab"] + outs["cw"] + outs["cb"] + [outs["gls"], outs["stats"], ws]
    assert all(bool((t == SENT).all()) for t in every)  # no refused call wrote anything: not an output, not the workspace
    call(logp_old=b["advantages"].data_ptr())()  # (inputs may share bytes with one another)
    call()()  # (the unedited call runs, and gives the engine's bits)
    torch.cuda.synchronize()
    want, want_gls, want_stats = fused(eng, actor, critic, log_std, b, "tanh")
    for u, v in zip(outs["aw"] + outs["ab"] + outs["cw"] + outs["cb"], [want[i] for i in (0, 2, 4, 1, 3, 5, 6, 8, 7, 9)]):
        assert torch.equal(u, v)
    assert torch.equal(outs["gls"], want_gls) and torch.equal(outs["stats"][:9], want_stats[:9])
    with pytest.raises(ValueError, match="x must be a contiguous float32 tensor"):
        eng.ppo_grad(b["x"].cpu(), la, lc, log_std.detach(), b["actions"], b["logp_old"], b["advantages"], b["returns"])  # (a host tensor)


# ---------------------------------------------------------------------------------------------- 6. what is left in .grad
def test_grad_semantics_and_an_optimiser_step(eng):
    c = case(1000, 0, "quarter")
    actor, critic, log_std, b = on_device(c)
    batch = (b["actions"], b["logp_old"], b["advantages"], b["returns"])
    ps = params_of(actor, critic, log_std)
    assert all(p.grad is None for p in ps)
    stats = pyflyt_amd.ppo_grad(eng, b["x"], actor, critic, log_std, *batch, valid=b["valid"], **COEF)
    assert stats.shape == (16,) and stats.dtype == torch.float64 and b["x"].grad is None
    once = [p.grad.clone() for p in ps]  # (assigned where .grad was None, log_std's included)
    want, want_gls, want_stats, _, _ = composed(eng, actor, critic, log_std, b)
    for g, w in zip(once, want + [want_gls]):
        assert torch.equal(g, w)
    for p, g in zip(ps, once):
        p.grad = g.clone()
    held = [p.grad for p in ps]
    pyflyt_amd.ppo_grad(eng, b["x"], actor, critic, log_std, *batch, valid=b["valid"], **COEF)
    for p, h, g in zip(ps, held, once):
        assert p.grad is h and torch.equal(p.grad, g + g)  # (added to the tensor that was there)
    assert pyflyt_amd.ppo_stats_dict(stats)["valid_rows"] == int(b["valid"].sum())
    # the list form with activation=, a frozen parameter, an input that asks for a gradient
    for p in ps:
        p.grad = None
    critic[0].bias.requires_grad_(False)
    pyflyt_amd.ppo_grad(eng, b["x"], [(m.weight, m.bias) for m in actor if isinstance(m, torch.nn.Linear)], critic, log_std, *batch, valid=b["valid"],
                        activation="tanh", **COEF)
    assert critic[0].bias.grad is None and all(torch.equal(p.grad, g) for p, g in zip(ps, once) if p is not critic[0].bias)
    critic[0].bias.requires_grad_(True)
    with pytest.raises(ValueError, match="no gradient for x"):
        pyflyt_amd.ppo_grad(eng, b["x"].clone().requires_grad_(), actor, critic, log_std, *batch, **COEF)
    # one optimiser step on each path from the same parameters
    a2, c2, l2 = copy.deepcopy(actor), copy.deepcopy(critic), torch.nn.Parameter(log_std.detach().clone())
    p2 = params_of(a2, c2, l2)
    o1, o2 = pyflyt_amd.Adam(eng, ps, lr=3e-4, max_grad_norm=0.5), pyflyt_amd.Adam(eng, p2, lr=3e-4, max_grad_norm=0.5)
    for _ in range(2):
        o1.zero_grad()
        pyflyt_amd.ppo_grad(eng, b["x"], actor, critic, log_std, *batch, valid=b["valid"], **COEF)
        o1.step()
        loss, _ = pyflyt_amd.ppo_loss(eng, pyflyt_amd.mlp(eng, b["x"], a2), l2, pyflyt_amd.mlp(eng, b["x"], c2), *batch, valid=b["valid"], **COEF)
        o2.zero_grad()
        loss.backward()
        o2.step()
    for u, v in zip(ps, p2):
        assert torch.equal(u, v)


# ---------------------------------------------------------------------------------------------- 7. the example
def test_example_13_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "13_ppo_fused_epoch.py"), "256", "2"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("iteration")]
    assert len(lines) == 2 and "nan" not in out.stdout.lower() and "inf" not in out.stdout.lower()

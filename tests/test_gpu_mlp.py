"""pf_mlp_forward / pf_mlp_backward on the device: the forward is pf_policy_act's mean bit for bit; forward and parameter gradients
against torch autograd in float64 at the shapes where the tiling can go wrong; determinism over streams and repetitions; zero-gradient
rows and the ragged last tile; the autograd wrapper under ppo_loss; graph capture; refusals; the example."""
import copy
import ctypes as C
import math
import os
import subprocess
import sys

import pytest
import torch

import pyflyt_amd
from pyflyt_amd import MLPPolicy, PyFlytAmdError, build_params
from pyflyt_amd import _lib as L
from pyflyt_amd.engine import BatchEngine
from test_gpu_ppo_loss import CLIP, HALF_LOG_2PI, SHIFTS, hand_written_loss, inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETS = [((64, 64), "tanh"), ((33, 64), "relu"), ((1,), "tanh"), ((64, 1), "tanh")]


@pytest.fixture(scope="module")
def eng():
    """A context WITHOUT an env task: the calls use a context for its device and its error string only."""
    e = BatchEngine(build_params("quadx", "none"), 64, device=DEV)
    yield e
    e.close()


def make_layers(in_dim, hidden, out_dim, seed=5, scale=0.4):
    g = torch.Generator().manual_seed(seed)
    sizes = [in_dim, *hidden, out_dim]
    return [((torch.randn(o, i, generator=g) * scale / math.sqrt(i) * 3.0).to(DEV).contiguous(), (torch.randn(o, generator=g) * 0.1).to(DEV))
            for i, o in zip(sizes[:-1], sizes[1:])]


def grid_cap(eng, layers):
    """The most workgroups the backward takes, from the workspace size: a block of one float per parameter and workgroup."""
    q = eng._mlp_block(torch.zeros(1, layers[0][0].shape[1], device=DEV), layers, "tanh")[0]
    P = sum(w.numel() + b.numel() for w, b in layers)
    top = eng.lib.pf_mlp_backward_workspace_bytes(C.byref(q), 1 << 24)
    assert top % (4 * P) == 0
    return top // (4 * P)


def torch_reference(x, layers, activation, grad_out, dtype):
    """(out, [(grad_w, grad_b), ...]) by torch autograd in `dtype`, returned as float64."""
    ps = [(w.detach().to(dtype).requires_grad_(), b.detach().to(dtype).requires_grad_()) for w, b in layers]
    h = x.to(dtype)
    for l, (w, b) in enumerate(ps):
        h = h @ w.T + b
        if l + 1 < len(ps):
            h = torch.tanh(h) if activation == "tanh" else torch.relu(h)
    h.backward(grad_out.to(dtype))
    return h.detach().double(), [(w.grad.double(), b.grad.double()) for w, b in ps]


def bound_ratio(got, ref, f32):
    """err / max(e32, 2^-24 max|ref|): the test's bound is 8."""
    err = float((got.double() - ref).abs().max())
    e32 = float((f32 - ref).abs().max())
    return err / max(e32, 2.0 ** -24 * float(ref.abs().max()), 1e-300)


# ---------------------------------------------------------------------------------------------- 1. the forward is pf_policy_act's mean
@pytest.mark.parametrize("kind", ["hover", "dogfight"])
def test_forward_is_policy_act_mean(eng, kind):
    n = 1000
    if kind == "hover":
        env_eng = BatchEngine(build_params("quadx", "hover", seed=11), n, device=DEV)
    else:
        env_eng = BatchEngine(build_params("fixedwing", "dogfight", seed=11, autoreset="off", angle_representation="euler", vehicle_options=dict(drone_model="acrowing"),
                                           dogfight=dict(team_size=4, assisted_flight=False)), n, device=DEV)
    D, A = env_eng.obs_dim, env_eng.action_dim
    assert (D, A) == ((21, 4) if kind == "hover" else (123, 6))
    obs = env_eng.env_reset().clone()
    for hidden, activation in NETS:
        layers = make_layers(D, hidden, A)
        mean = torch.full((n, A), float("nan"), device=DEV)
        env_eng.policy_act(MLPPolicy(layers, activation=activation, log_std=None), obs=obs, mean_out=mean)
        out = eng.mlp_forward(obs, layers, activation, out=torch.full((n, A), float("nan"), device=DEV))
        assert torch.isfinite(mean).all() and torch.equal(out, mean), (kind, hidden, activation)
        assert torch.equal(env_eng.mlp_forward(obs, layers, activation), mean)  # (any context: one with an env task as well)
    env_eng.close()


# ---------------------------------------------------------------------------------------------- 2. shapes, against float64
# rows: one row, one short of a tile, a tile, a tile and a row, two tiles and a row; MANY = more tiles than the grid has workgroups.
# in_dim: 1, 21, 35 (odd: a zero last k-pair), 64 (one full chunk), 65 (a second chunk of one column), 123. out_dim 1, 4, 7. Widths
# 64 / 33 / 1. ReLU only at the small row counts: its derivative jumps at 0, and over 2 M hidden activations one within rounding of 0
# in float32 but on the other side in float64 is likely (about 1 in 10 per million), which no rounding bound covers -- for torch neither.
MANY = "many"
SHAPES = [
    (1, 21, (64, 64), 4, "tanh"),
    (63, 1, (64,), 1, "tanh"),
    (64, 35, (33, 64), 7, "relu"),
    (65, 64, (64, 33), 4, "tanh"),
    (129, 65, (1,), 1, "relu"),
    (129, 123, (64, 64), 7, "tanh"),
    (129, 21, (64, 1), 4, "relu"),
    (65, 21, (64,), 1, "relu"),
    (MANY, 21, (64, 64), 4, "tanh"),
    (MANY, 65, (33,), 1, "tanh"),
]


@pytest.mark.parametrize("rows, in_dim, hidden, out_dim, activation", SHAPES)
def test_against_float64(eng, rows, in_dim, hidden, out_dim, activation):
    layers = make_layers(in_dim, hidden, out_dim, seed=in_dim + out_dim)
    if rows == MANY:
        cap = grid_cap(eng, layers)
        rows = 64 * (2 * cap + 1) + 37  # every workgroup accumulates over two tiles or more; the sum over the workgroups has `cap` terms
        assert eng.lib.pf_mlp_backward_workspace_bytes(C.byref(eng._mlp_block(torch.zeros(rows, in_dim, device=DEV), layers, activation)[0]), rows) \
            == 4 * cap * sum(w.numel() + b.numel() for w, b in layers)
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, in_dim, generator=g).to(DEV)
    grad_out = (torch.randn(rows, out_dim, generator=g) * 0.1).to(DEV)
    out64, g64 = torch_reference(x, layers, activation, grad_out, torch.float64)
    out32, g32 = torch_reference(x, layers, activation, grad_out, torch.float32)
    out = eng.mlp_forward(x, layers, activation)
    grads = eng.mlp_backward(x, grad_out, layers, activation)
    ratios = {"out": bound_ratio(out, out64, out32)}
    for l, ((gw, gb), (rw, rb), (fw, fb)) in enumerate(zip(grads, g64, g32)):
        assert gw.shape == layers[l][0].shape and gb.shape == layers[l][1].shape
        ratios[f"grad_w[{l}]"] = bound_ratio(gw, rw, fw)
        ratios[f"grad_b[{l}]"] = bound_ratio(gb, rb, fb)
    print(f"rows {rows} in {in_dim} hidden {hidden} out {out_dim} {activation}: err / max(e32, 2^-24 max|ref|): " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(float(r[0].abs().max()) > 0 for r in g64)
    for k, v in ratios.items():
        assert v <= 8.0, (k, v)


# ---------------------------------------------------------------------------------------------- 3. determinism
def test_same_bits_on_every_stream_and_repetition(eng):
    layers = make_layers(21, (64, 64), 4)
    rows = 64 * (grid_cap(eng, layers) + 3) + 5
    g = torch.Generator().manual_seed(1)
    x, grad_out = torch.randn(rows, 21, generator=g).to(DEV), torch.randn(rows, 4, generator=g).to(DEV)
    first = [t.clone() for pair in eng.mlp_backward(x, grad_out, layers, "tanh") for t in pair]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        second = [t.clone() for pair in eng.mlp_backward(x, grad_out, layers, "tanh") for t in pair]
    side.synchronize()
    third = [t.clone() for pair in eng.mlp_backward(x, grad_out, layers, "tanh") for t in pair]
    for a, b, c in zip(first, second, third):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert all(float(a.abs().sum()) > 0 for a in first)


# ---------------------------------------------------------------------------------------------- 4. masked rows
@pytest.mark.parametrize("hidden, activation", [((64, 64), "tanh"), ((33,), "relu")])
def test_zero_gradient_rows_contribute_exact_zeros(eng, hidden, activation):
    """A quarter of the rows have a +0 gradient: tile 1 whole (rows 64 .. 127), and a few rows of tile 2 (mixed). What their x holds
    -- as long as it is finite -- changes no bit."""
    rows, D, A = 64 * 4 + 17, 21, 4
    layers = make_layers(D, hidden, A)
    g = torch.Generator().manual_seed(2)
    x, grad_out = torch.randn(rows, D, generator=g).to(DEV), torch.randn(rows, A, generator=g).to(DEV)
    zero = torch.zeros(rows, dtype=torch.bool, device=DEV)
    zero[64:128] = True
    zero[[130, 137, 150, 191]] = True
    assert abs(int(zero.sum()) - rows // 4) <= 1
    grad_out[zero] = 0.0
    a = [t.clone() for pair in eng.mlp_backward(x, grad_out, layers, activation) for t in pair]
    x2 = x.clone()
    x2[zero] = (torch.randn(int(zero.sum()), D, generator=g) * 50.0).to(DEV)
    b = [t.clone() for pair in eng.mlp_backward(x2, grad_out, layers, activation) for t in pair]
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert all(float(u.abs().sum()) > 0 for u in a)


def test_ragged_last_tile_reads_nothing_past_its_rows(eng):
    """The NaN lies past `rows`, in a larger allocation the call is told nothing about: the last tile masks, it does not read."""
    rows, D, A = 70, 35, 4
    layers = make_layers(D, (64, 64), A)
    g = torch.Generator().manual_seed(3)
    xbig = torch.full((rows + 64, D), float("nan"), device=DEV)
    gbig = torch.full((rows + 64, A), float("nan"), device=DEV)
    xbig[:rows], gbig[:rows] = torch.randn(rows, D, generator=g).to(DEV), torch.randn(rows, A, generator=g).to(DEV)
    got = [t.clone() for pair in eng.mlp_backward(xbig[:rows], gbig[:rows], layers, "tanh") for t in pair]
    out = eng.mlp_forward(xbig[:rows], layers, "tanh").clone()
    assert all(torch.isfinite(t).all() for t in got) and torch.isfinite(out).all()
    want = [t.clone() for pair in eng.mlp_backward(xbig[:rows].clone(), gbig[:rows].clone(), layers, "tanh") for t in pair]
    for u, v in zip(got, want):
        assert torch.equal(u, v)


# ---------------------------------------------------------------------------------------------- 5. autograd
def test_autograd_under_ppo_loss(eng):
    M, A, D = 1000, 4, 21
    vf_coef, ent_coef = 0.5, 0.0078125
    g = torch.Generator().manual_seed(5)
    obs = torch.randn(M, D, generator=g).to(DEV)
    nn = torch.nn
    torch.manual_seed(11)
    actor = nn.Sequential(nn.Linear(D, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, A)).to(DEV)
    critic = nn.Sequential(nn.Linear(D, 64), nn.Tanh(), nn.Linear(64, 1)).to(DEV)
    log_std = nn.Parameter(torch.linspace(-0.8, 0.2, A, device=DEV))
    with torch.no_grad():  # (test_gpu_ppo_loss's batch: ratios away from the clip bounds under THIS actor)
        mean = actor(obs)
        gi = torch.Generator().manual_seed(6)
        z = ((torch.rand(M, A, generator=gi, dtype=torch.float64) * 2.0 - 1.0) * 3.9).to(DEV)
        actions = (mean.double() + z * log_std.double().exp()).float()
        zz = (actions.double() - mean.double()) * (-log_std.double()).exp()
        logp = (-0.5 * zz * zz - log_std.double() - HALF_LOG_2PI).sum(-1)
        d = torch.tensor(SHIFTS, dtype=torch.float64)[torch.randint(0, 5, (M,), generator=gi)].to(DEV)
        base = inputs(M, A)
        x = dict(actions=actions, logp_old=(logp - d).float(), advantages=base["advantages"], returns=base["returns"], valid=base["valid"])
    actor64, critic64, log_std64 = copy.deepcopy(actor).double(), copy.deepcopy(critic).double(), nn.Parameter(log_std.detach().double())

    def grads(params):
        out = [p.grad.double().clone() for p in params]
        for p in params:
            p.grad = None
        return out

    p32 = list(actor.parameters()) + list(critic.parameters()) + [log_std]
    p64 = list(actor64.parameters()) + list(critic64.parameters()) + [log_std64]
    hand_written_loss(actor64, critic64, log_std64, obs, x, torch.float64, vf_coef, ent_coef).backward()
    g64 = grads(p64)
    hand_written_loss(actor, critic, log_std, obs, x, torch.float32, vf_coef, ent_coef).backward()
    g32 = grads(p32)
    out_a, out_c = pyflyt_amd.mlp(eng, obs, actor), pyflyt_amd.mlp(eng, obs, critic)
    assert out_a.shape == (M, A) and out_c.shape == (M, 1) and out_a.requires_grad and out_c.requires_grad
    loss, _ = pyflyt_amd.ppo_loss(eng, out_a, log_std, out_c, x["actions"], x["logp_old"], x["advantages"], x["returns"], valid=x["valid"], clip=CLIP,
                                  vf_coef=vf_coef, ent_coef=ent_coef, normalize_advantage=True)
    loss.backward()
    assert all(p.grad is not None for p in p32) and obs.grad is None
    ours = grads(p32)
    names = [f"actor.{n}" for n, _ in actor.named_parameters()] + [f"critic.{n}" for n, _ in critic.named_parameters()] + ["log_std"]
    ratios = {}
    for name, got, ref, f32 in zip(names, ours, g64, g32):
        ratios[name] = float((got - ref).abs().max()) / max(float((f32 - ref).abs().max()), 2.0 ** -24 * float(ref.abs().max()))
    print("autograd: err / max(e32, 2^-24 max|ref|): " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 8.0 for v in ratios.values()), ratios
    # the list form, and an input that asks for a gradient
    pairs = [(actor[0].weight, actor[0].bias), (actor[2].weight, actor[2].bias), (actor[4].weight, actor[4].bias)]
    assert torch.equal(pyflyt_amd.mlp(eng, obs, pairs, activation="tanh"), out_a)
    with pytest.raises(ValueError, match="no gradient for x"):
        pyflyt_amd.mlp(eng, obs.clone().requires_grad_(), actor)


# ---------------------------------------------------------------------------------------------- 6. capture
def test_forward_and_backward_are_capturable(eng):
    rows, D, A = 64 * 5 + 9, 21, 4
    layers = make_layers(D, (64, 64), A)
    g = torch.Generator().manual_seed(4)
    x, grad_out = torch.randn(rows, D, generator=g).to(DEV), torch.randn(rows, A, generator=g).to(DEV)
    out = eng.mlp_forward(x, layers, "tanh")
    grads = eng.mlp_backward(x, grad_out, layers, "tanh")  # (the engine's tensors for this shape exist from here on)
    eager = [out.clone()] + [t.clone() for pair in grads for t in pair]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        before = torch.cuda.memory_allocated(DEV)
        out2 = eng.mlp_forward(x, layers, "tanh")
        grads2 = eng.mlp_backward(x, grad_out, layers, "tanh")
        assert torch.cuda.memory_allocated(DEV) == before
    assert out2 is out and all(a is b for p, q in zip(grads, grads2) for a, b in zip(p, q))
    for _ in range(2):
        for t in [out] + [t for pair in grads for t in pair]:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for want, got in zip(eager, [out] + [t for pair in grads for t in pair]):
            assert torch.equal(want, got)


# ---------------------------------------------------------------------------------------------- 7. arguments
def _raises(fragment, fn):
    with pytest.raises(PyFlytAmdError) as e:
        fn()
    assert e.value.code == L.ERR_ARG and fragment in str(e.value), str(e.value)


def test_refusals_name_the_argument(eng):
    rows, D, A = 100, 21, 4
    layers = make_layers(D, (16, 8), A)
    x, grad_out, out = torch.zeros(2 * rows, D, device=DEV), torch.zeros(2 * rows, A, device=DEV), torch.zeros(rows, A, device=DEV)
    q0 = eng._mlp_block(x[:rows], layers, "tanh")[0]
    need = eng.lib.pf_mlp_backward_workspace_bytes(C.byref(q0), rows)
    assert need == 4 * 2 * sum(w.numel() + b.numel() for w, b in layers)
    ws = torch.zeros(need // 4, device=DEV)
    gtens = [(torch.zeros_like(w), torch.zeros_like(b)) for w, b in layers]

    def call(edit=None, forward=False, **kw):
        q = eng._mlp_block(x[:rows], layers, "tanh")[0]
        if edit:
            edit(q)
        a = dict(ctx=eng._ctx, q=C.byref(q), x=x.data_ptr(), grad_out=grad_out.data_ptr(), out=out.data_ptr(), rows=rows, ws=ws.data_ptr(), bytes=need,
                 gw=[t[0].data_ptr() for t in gtens], gb=[t[1].data_ptr() for t in gtens])
        a.update(kw)
        gw = (C.c_void_p * 3)(*a["gw"]) if a["gw"] is not None else None
        gb = (C.c_void_p * 3)(*a["gb"]) if a["gb"] is not None else None
        if forward:
            return lambda: L.check(eng.lib.pf_mlp_forward(a["ctx"], a["q"], a["x"], a["rows"], a["out"], eng._stream()), a["ctx"])
        return lambda: L.check(eng.lib.pf_mlp_backward(a["ctx"], a["q"], a["x"], a["grad_out"], a["rows"], gw, gb, a["ws"], a["bytes"], eng._stream()), a["ctx"])

    def setter(name, value, index=None):
        def edit(q):
            if index is None:
                setattr(q, name, value)
            else:
                getattr(q, name)[index] = value
        return edit

    for fwd in (True, False):
        who = "pf_mlp_forward" if fwd else "pf_mlp_backward"
        _raises(f"{who}: ctx is required", call(forward=fwd, ctx=None))
        _raises(f"{who}: mlp is required", call(forward=fwd, q=None))
        _raises(f"{who}: x is required", call(forward=fwd, x=None))
        _raises(f"{who}: rows must be >= 1", call(forward=fwd, rows=0))
        _raises(f"{who}: rows must be >= 1", call(forward=fwd, rows=-5))
        _raises(f"{who}: rows must be below", call(forward=fwd, rows=(1 << 31) - 64))
        _raises(f"{who}: n_layers must be 2 or 3", call(setter("n_layers", 1), forward=fwd))
        _raises(f"{who}: n_layers must be 2 or 3", call(setter("n_layers", 4), forward=fwd))
        _raises(f"{who}: width", call(setter("width", 0, 0), forward=fwd))
        _raises(f"{who}: width", call(setter("width", 65, 1), forward=fwd))
        _raises(f"{who}: in_dim must be in 1..128", call(setter("in_dim", 0), forward=fwd))
        _raises(f"{who}: in_dim must be in 1..128", call(setter("in_dim", 129), forward=fwd))
        _raises(f"{who}: out_dim must be in 1..8", call(setter("out_dim", 0), forward=fwd))
        _raises(f"{who}: out_dim must be in 1..8", call(setter("out_dim", 9), forward=fwd))
        _raises(f"{who}: activation must be", call(setter("activation", 2), forward=fwd))
        _raises(f"{who}: w / b", call(setter("w", None, 1), forward=fwd))
        _raises(f"{who}: w / b", call(setter("b", None, 2), forward=fwd))
    _raises("pf_mlp_forward: out is required", call(forward=True, out=None))
    _raises("pf_mlp_forward: x and out overlap", call(forward=True, out=x.data_ptr() + 4 * (rows * D - 1)))
    _raises("pf_mlp_backward: grad_out is required", call(grad_out=None))
    _raises("pf_mlp_backward: grad_w is required", call(gw=None))
    _raises("pf_mlp_backward: grad_b is required", call(gb=None))
    _raises("pf_mlp_backward: grad_w:", call(gw=[gtens[0][0].data_ptr(), None, gtens[2][0].data_ptr()]))
    _raises("pf_mlp_backward: grad_b:", call(gb=[gtens[0][1].data_ptr(), gtens[1][1].data_ptr(), None]))
    _raises("pf_mlp_backward: workspace is required", call(ws=None))
    _raises("pf_mlp_backward: workspace_bytes", call(bytes=need - 1))  # (refused by size: the buffer itself is large enough)
    _raises("pf_mlp_backward: workspace_bytes", call(bytes=0))
    _raises("pf_mlp_backward: x and grad_out overlap", call(grad_out=x.data_ptr() + 4 * D))
    _raises("pf_mlp_backward: x and workspace overlap", call(ws=x.data_ptr() + 4 * D * (rows - 1)))
    _raises("pf_mlp_backward: grad_out and grad_w[0] overlap", call(gw=[grad_out.data_ptr(), gtens[1][0].data_ptr(), gtens[2][0].data_ptr()]))
    _raises("pf_mlp_backward: workspace and grad_b[2] overlap", call(gb=[gtens[0][1].data_ptr(), gtens[1][1].data_ptr(), ws.data_ptr() + need - 4]))
    _raises("pf_mlp_backward: grad_w[1] and grad_b[1] overlap", call(gb=[gtens[0][1].data_ptr(), gtens[1][0].data_ptr(), gtens[2][1].data_ptr()]))
    call(forward=True)()  # (the unedited calls run)
    call()()
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="x must be a contiguous float32 tensor"):
        eng.mlp_forward(torch.zeros(rows, D), layers, "tanh")  # (a host tensor)


# ---------------------------------------------------------------------------------------------- 8. the example
def test_example_10_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "10_ppo_on_device_networks.py"), "256", "2"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "iteration 1" in out.stdout

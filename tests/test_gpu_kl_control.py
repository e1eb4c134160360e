"""pf_kl_control and pf_adam_step_gated on the device: the KL decisions of a PPO recipe without a host read.

Exact checks only: the control's comparisons are in double on widened float32 arguments and its two learning-rate operations are
single float32 operations, so a host restatement in the same formats gives the same bits; a gated step with an open gate is
pf_adam_step, and with a closed one it changes nothing but its counters."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pyflyt_amd
from pyflyt_amd import MLPPolicy, PyFlytAmdError, build_params
from pyflyt_amd import _lib as L
from pyflyt_amd.engine import BatchEngine
from pyflyt_amd.gym_envs import make_vec
from test_gpu_adam import EX10, Ours, draws
from test_gpu_ppo_grad import layers_of, sequential
from test_gpu_ppo_loss import f32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def eng():
    e = BatchEngine(build_params("quadx", "none"), 64, device=DEV)
    yield e
    e.close()


def control(eng, kl, lr, adapt=True, target=0.01, stop=1.5, state=None, **kw):
    stats = torch.zeros(16, dtype=torch.float64, device=DEV)
    stats[5] = kl
    gate = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    state = torch.zeros(4, dtype=torch.float64, device=DEV) if state is None else state
    lr_t = None if lr is None else torch.full((1,), lr, device=DEV)
    eng.kl_control(stats, gate, state, target, stop, lr=lr_t, adapt=adapt, **kw)
    torch.cuda.synchronize()
    return int(gate), (None if lr_t is None else lr_t.cpu().numpy()[0]), state


def test_learning_rate_and_gate_against_a_host_float32_computation(eng):
    kw = dict(factor=1.5, low=0.5, high=2.0, lr_min=1e-5, lr_max=1e-3)
    t = float(F(0.01))
    lr0 = F(3e-4)
    cases = [(0.5 * t * 0.99, "raise"), (0.5 * t, "keep"), (t, "keep"), (2.0 * t, "keep"), (2.0 * t * 1.01, "cut"), (math.nan, "keep"), (math.inf, "cut"), (-1e-9, "raise")]
    for kl, what in cases:
        gate, lr, state = control(eng, kl, float(lr0), **kw)
        want = {"raise": min(F(lr0 * F(1.5)), F(1e-3)), "cut": max(F(lr0 / F(1.5)), F(1e-5)), "keep": lr0}[what]
        assert lr.tobytes() == F(want).tobytes(), (kl, what, lr, want)
        assert gate == (1 if kl <= float(F(1.5)) * t else 0), (kl, gate)
        st = state.tolist()
        assert (math.isnan(st[0]) if math.isnan(kl) else st[0] == kl) and st[1] == float(lr) and st[2] == gate and st[3] == 1 - gate
    # the clamps
    _, lr, _ = control(eng, 0.0, 9e-4, **kw)
    assert lr.tobytes() == F(1e-3).tobytes()
    _, lr, _ = control(eng, 1.0, 1.2e-5, **kw)
    assert lr.tobytes() == F(1e-5).tobytes()
    # adapt = 0: the bits of lr are untouched, and the state reports it; no lr at all: 0
    odd = float(np.frombuffer(np.uint32(0x3A83126F + 3).tobytes(), dtype=F)[0])
    gate, lr, state = control(eng, 1.0, odd, adapt=False)
    assert lr.tobytes() == F(odd).tobytes() and gate == 0 and state.tolist() == [1.0, odd, 0.0, 1.0]
    gate, lr, state = control(eng, 0.001, None, adapt=False)
    assert gate == 1 and state.tolist() == [0.001, 0.0, 1.0, 0.0]
    # stop_factor = inf closes on a NaN only; the count runs on
    state = torch.zeros(4, dtype=torch.float64, device=DEV)
    seen = [control(eng, kl, None, adapt=False, stop=math.inf, state=state)[0] for kl in (1e30, math.inf, math.nan, math.nan, 0.0)]
    assert seen == [1, 1, 0, 0, 1] and state.tolist()[2:] == [1.0, 2.0]


def test_control_refusals_name_the_argument(eng):
    stats, gate, state = torch.zeros(16, dtype=torch.float64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(4, dtype=torch.float64, device=DEV)
    lr = torch.full((1,), 1e-3, device=DEV)
    import ctypes as C

    def run(**kw):
        a = L.PfKlControl()
        a.stats, a.gate, a.state, a.lr_dev = stats.data_ptr(), gate.data_ptr(), state.data_ptr(), lr.data_ptr()
        a.target_kl, a.stop_factor, a.adapt, a.lr_factor, a.lr_low, a.lr_high, a.lr_min, a.lr_max = 0.01, 1.5, 1, 1.5, 0.5, 2.0, 1e-6, 1e-2
        for k, v in kw.items():
            setattr(a, k, v)
        with pytest.raises(PyFlytAmdError) as e:
            L.check(eng.lib.pf_kl_control(eng._ctx, C.byref(a), eng._stream()), eng._ctx)
        assert e.value.code == L.ERR_ARG
        return str(e.value)

    for name in ("stats", "gate", "state"):
        assert f"pf_kl_control: {name} is required" in run(**{name: None})
    for kw, text in ((dict(target_kl=0.0), "target_kl"), (dict(target_kl=math.inf), "target_kl"), (dict(stop_factor=0.99), "stop_factor"), (dict(stop_factor=math.nan), "stop_factor"),
                     (dict(adapt=2), "adapt must be 0 or 1"), (dict(lr_dev=None), "lr_dev is required"), (dict(lr_factor=1.0), "lr_factor"), (dict(lr_low=2.0), "lr_low"),
                     (dict(lr_low=0.0), "lr_low"), (dict(lr_min=0.0), "lr_min"), (dict(lr_max=1e-7), "lr_min"), (dict(lr_max=math.inf), "lr_max"),
                     (dict(gate=state.data_ptr()), "gate"), (dict(lr_dev=stats.data_ptr() + 8), "lr_dev")):
        assert text in run(**kw), (kw, text)


class Gated(Ours):
    """test_gpu_adam.py's Ours with a gate the test sets."""

    def __init__(self, eng, p0, unaligned=False, **hp):
        super().__init__(eng, p0, unaligned, **hp)
        self.eng, self.gate = eng, torch.ones(1, dtype=torch.int32, device=DEV)

    def step(self, grads, gate=1):
        for t, g in zip(self.grads, grads):
            t.copy_(g)
        self.gate.fill_(gate)
        o = self.opt
        self.eng.adam_step(self.params, self.grads, o.exp_avg, o.exp_avg_sq, o.state, lr=o.lr, betas=o.betas, eps=o.eps, weight_decay=o.weight_decay,
                           max_grad_norm=o.max_grad_norm, skip_nonfinite=o.skip_nonfinite, gate=self.gate)
        return o.state.clone()


@pytest.mark.parametrize("unaligned", (False, True))
def test_gated_adam_over_eleven_tensors(eng, unaligned):
    p0, grads = draws(EX10, steps=3)
    hp = dict(lr=1e-2, weight_decay=0.01, max_grad_norm=0.05, skip_nonfinite=True)
    plain, gated = Ours(eng, p0, unaligned, **hp), Gated(eng, p0, unaligned, **hp)
    for g in grads[:2]:  # gate 1 is pf_adam_step: parameters, moments and state
        assert torch.equal(plain.step(g), gated.step(g, 1))
    for xs, ys in zip(plain.result(), gated.result()):
        assert all(torch.equal(x, y) for x, y in zip(xs, ys)) if isinstance(xs, list) else torch.equal(xs, ys)
    before = gated.result()
    s = gated.step(grads[2], 0)  # gate 0: nothing moves but the counters
    for xs, ys in zip(before[:3], gated.result()[:3]):
        assert all(torch.equal(x, y) for x, y in zip(xs, ys))
    norm = math.sqrt(sum(float(g.double().pow(2).sum()) for g in grads[2]))
    st = s.tolist()
    assert st[0] == 2.0 and abs(st[1] - norm) <= 1e-12 * norm and st[2] == 0.0 and st[4] == 0.0 and st[5] == 1.0 and st[6:] == [0.0, 0.0]
    s = gated.step(grads[2], 0)
    assert s.tolist()[5] == 2.0 and s.tolist()[0] == 2.0
    s = gated.step(grads[2], 1)  # a closed gate followed by an open one is one plain step
    want = plain.step(grads[2])
    assert torch.equal(s[:5], want[:5]) and s.tolist()[5] == 2.0
    for xs, ys in zip(plain.result()[:3], gated.result()[:3]):
        assert all(torch.equal(x, y) for x, y in zip(xs, ys))
    # a norm that is not finite under a closed gate: both are counted, nothing moves
    bad = [g.clone() for g in grads[0]]
    bad[2][17, 5] = float("inf")
    before = gated.result()
    s = gated.step(bad, 0).tolist()
    assert s[0] == 3.0 and s[2] == 0.0 and s[4] == 1.0 and s[5] == 3.0
    for xs, ys in zip(before[:3], gated.result()[:3]):
        assert all(torch.equal(x, y) for x, y in zip(xs, ys))
    with pytest.raises(PyFlytAmdError, match="pf_adam_step_gated: .*gate"):
        gated.eng.adam_step(gated.params, gated.grads, gated.opt.exp_avg, gated.opt.exp_avg_sq, gated.opt.state, gate=gated.opt.state.view(torch.int32)[4:5])


def test_early_stop_end_to_end_and_in_one_graph():
    env = make_vec("PyFlyt/QuadX-Hover-v4", num_envs=256, device=DEV, seed=11)
    try:
        env.reset(seed=11)
        eng = env.engine
        D, A = env.single_observation_space.shape[0], env.single_action_space.shape[0]
        torch.manual_seed(3)
        actor, critic = sequential([D, 64, 64, A], "tanh").to(DEV), sequential([D, 64, 1], "tanh").to(DEV)
        log_std = torch.full((A,), -0.5, device=DEV)
        batch = env.collect(MLPPolicy.from_torch(actor, log_std=log_std), critic, 16)
        b = {k: (batch[k].reshape(-1, batch[k].shape[-1]) if k in ("obs", "actions") else batch[k].reshape(-1)).clone()
             for k in ("obs", "actions", "logp", "advantages", "returns", "valid", "values")}
        la, lc = layers_of(actor), layers_of(critic)
        params = [t for pair in la for t in pair] + [t for pair in lc for t in pair] + [log_std]
        start = [p.clone() for p in params]
        opts = dict(clip_vf=0.2, values_old=b["values"], action_bounds=(env.single_action_space.low, env.single_action_space.high), bounds_coef=1e-4)

        def epoch(opt, gated):
            ga, gc, gls, stats = eng.ppo_grad(b["obs"], la, lc, log_std, b["actions"], b["logp"], b["advantages"], b["returns"], valid=b["valid"], **opts)
            grads = [t for pair in ga for t in pair] + [t for pair in gc for t in pair] + [gls]
            opt.step(grads=grads, stats=stats) if gated else opt.step(grads=grads)
            return stats

        # what the first two epochs measure, with a plain optimiser; the parameters after ONE step
        plain = pyflyt_amd.Adam(eng, params, lr=3e-3, max_grad_norm=0.5)
        kl1 = float(epoch(plain, False)[5])
        after_one = [p.clone() for p in params]
        kl2 = float(epoch(plain, False)[5])
        assert kl2 > 0.0 and abs(kl1) < 0.25 * kl2, (kl1, kl2)
        target = 0.5 * kl2  # (with kl_stop = 1: the first epoch's KL is under it, the second's is over it)

        def run(replay):
            for p, s in zip(params, start):
                p.copy_(s)
            opt = pyflyt_amd.Adam(eng, params, lr=3e-3, max_grad_norm=0.5, target_kl=target, kl_stop=1.0)
            if replay:
                epoch(opt, True)  # the warm-up makes every cached block; then everything is put back
                for p, s in zip(params, start):
                    p.copy_(s)
                for t in opt.exp_avg + opt.exp_avg_sq + [opt.state, opt.kl_state]:
                    t.zero_()
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    for _ in range(4):
                        epoch(opt, True)
                graph.replay()
            else:
                for _ in range(4):
                    epoch(opt, True)
            torch.cuda.synchronize()
            return opt, [p.clone() for p in params], [t.clone() for t in opt.exp_avg + opt.exp_avg_sq + [opt.state, opt.kl_state, opt.gate]]

        opt, got, rest = run(False)
        d, s = opt.kl_dict(), opt.stats_dict()
        assert s["step"] == 1 and d["gated_steps"] == 3 and d["gated_calls"] == 3 and d["gate"] == 0 and d["approx_kl"] == kl2
        assert set(s) == {"step", "grad_norm", "clip_coef", "lr", "skipped"}
        for p, q in zip(got, after_one):
            assert torch.equal(p, q)
        _, got2, rest2 = run(True)
        for p, q in zip(got + rest, got2 + rest2):
            assert torch.equal(p, q)
    finally:
        env.close()


def test_example_16_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "16_ppo_recipe_options.py"), "256", "2"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l for l in out.stdout.splitlines() if l.startswith("iter")]
    assert len(lines) == 2 and all(k in lines[-1] for k in ("kl", "vclip", "bounds", "gated", "lr"))

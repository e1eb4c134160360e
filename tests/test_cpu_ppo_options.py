"""The host side of PPO's options (pf_ppo_loss_opt / pf_ppo_grad_opt), pf_kl_control and pf_adam_step_gated: the header's text, the
binding, the refusals of the C functions that need no device (a NULL ctx) and the argument checks of the Python layer."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from bare_engine import bare_engine
import pyflyt_amd
from pyflyt_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pf_sizeof_ppo_options", "pf_ppo_loss_opt", "pf_ppo_grad_opt", "pf_sizeof_kl_control", "pf_kl_control", "pf_adam_step_gated")


def test_header_states_the_contract():
    text = open(os.path.join(ROOT, "include", "pyflyt_amd.h")).read()
    assert re.search(r"typedef\s+struct\s+pf_ppo_options\s*\{", text) and re.search(r"typedef\s+struct\s+pf_kl_control_args\s*\{", text)
    assert re.search(r"int\s+pf_ppo_loss_opt\s*\(\s*pf_ctx\s*\*\s*\w+,\s*const\s+pf_ppo_loss_args\s*\*\s*\w+,\s*const\s+pf_ppo_options\s*\*\s*\w+,\s*size_t\s+rows,\s*int\s+width,"
                     r"\s*void\s*\*\s*stream\s*\)", text)
    assert re.search(r"int\s+pf_ppo_grad_opt\s*\(\s*pf_ctx\s*\*\s*\w+,\s*const\s+pf_ppo_grad_args\s*\*\s*\w+,\s*const\s+pf_ppo_options\s*\*\s*\w+,\s*int64_t\s+rows,", text)
    assert re.search(r"int\s+pf_kl_control\s*\(\s*pf_ctx\s*\*\s*\w+,\s*const\s+pf_kl_control_args\s*\*\s*\w+,\s*void\s*\*\s*stream\s*\)", text)
    assert re.search(r"int\s+pf_adam_step_gated\s*\(\s*pf_ctx\s*\*\s*\w+,\s*const\s+pf_adam_args\s*\*\s*\w+,\s*const\s+uint32_t\s*\*\s*gate,", text)
    contract = text.split("typedef struct pf_ppo_options")[0].rsplit("PPO's usual options", 1)[1]
    for fragment in ("OPTIONS OFF", "VALUE CLIPPING", "BOUNDS LOSS", "vc = e > 0 ? V_old + clip_vf : V_old - clip_vf", "use_c = out && dc^2 > dv^2",
                     "grad_value = use_c ? 0 : kv * dv", "hx = fmaxf(m_c - hi_c, 0)", "((2 * bounds_coef) * w32) * (hx - lx)", "stats[12]", "stats[13]"):
        assert fragment in contract, fragment
    assert "#define PF_ABI_VERSION 10" in text and L.PF_ABI_VERSION == 10
    for name in NAMES:
        assert name in L.EXPORTS


def test_struct_mirrors_match_the_library():
    assert [f[0] for f in L.PfPpoOptions._fields_] == ["clip_vf", "values_old", "bounds_coef", "bounds_lo", "bounds_hi"]
    assert C.sizeof(L.PfPpoOptions) == 8 + 8 + 4 + 2 * 8 * 4 + 4  # (clip_vf + padding; the pointer; bounds_coef; the bounds; tail padding)
    assert [f[0] for f in L.PfKlControl._fields_] == ["stats", "target_kl", "stop_factor", "adapt", "lr_factor", "lr_low", "lr_high", "lr_min", "lr_max",
                                                      "lr_dev", "gate", "state"]
    assert C.sizeof(L.PfKlControl) == 8 + 8 * 4 + 3 * 8
    if not os.path.exists(L.LIB_PATH):
        pytest.fail(f"{L.LIB_PATH} is not built")
    lib = C.CDLL(L.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name)
    lib.pf_sizeof_ppo_options.restype = lib.pf_sizeof_kl_control.restype = lib.pf_sizeof_ppo_loss.restype = lib.pf_sizeof_adam.restype = C.c_size_t
    assert lib.pf_sizeof_ppo_options() == C.sizeof(L.PfPpoOptions) and lib.pf_sizeof_kl_control() == C.sizeof(L.PfKlControl)
    assert lib.pf_sizeof_ppo_loss() == C.sizeof(L.PfPpoLoss) and lib.pf_sizeof_adam() == C.sizeof(L.PfAdam)  # (the existing blocks are as they were)


def test_c_functions_refuse_a_null_ctx():
    lib = L.lib()
    err = lambda: lib.pf_last_error(None).decode()  # noqa: E731
    o, a, g, k, ad = L.PfPpoOptions(), L.PfPpoLoss(), L.PfPpoGradArgs(), L.PfKlControl(), L.PfAdam()
    assert lib.pf_ppo_loss_opt(None, C.byref(a), C.byref(o), 8, 4, None) == L.ERR_ARG and err() == "pf_ppo_loss_opt: ctx and the argument block are required"
    assert lib.pf_ppo_loss(None, C.byref(a), 8, 4, None) == L.ERR_ARG and err() == "pf_ppo_loss: ctx and the argument block are required"
    assert lib.pf_ppo_grad_opt(None, C.byref(g), C.byref(o), 8, None, 0, None) == L.ERR_ARG and err() == "pf_ppo_grad_opt: ctx is required"
    assert lib.pf_kl_control(None, C.byref(k), None) == L.ERR_ARG and err() == "pf_kl_control: ctx is required"
    assert lib.pf_adam_step_gated(None, C.byref(ad), None, None, 0, None) == L.ERR_ARG and err() == "pf_adam_step_gated: ctx is required"


def test_stats_dict_key_counts():
    stats = torch.arange(16, dtype=torch.float64)
    d, e = pyflyt_amd.ppo_stats_dict(stats), pyflyt_amd.ppo_stats_dict(stats, options=True)
    assert len(d) == 12 and len(e) == 14 and list(e)[:12] == list(d)
    assert e["value_clip_fraction"] == 12.0 and e["bounds_loss"] == 13.0


def _loss_args(M=6, A=4):
    return dict(mean=torch.zeros(M, A), log_std=torch.zeros(A), value=torch.zeros(M), actions=torch.zeros(M, A), logp_old=torch.zeros(M),
                advantages=torch.zeros(M), returns=torch.zeros(M))


OPTION_REFUSALS = [
    (dict(clip_vf=0.2), "values_old is required with clip_vf"),
    (dict(values_old=torch.zeros(6)), "values_old comes with clip_vf"),
    (dict(clip_vf=0.0, values_old=torch.zeros(6)), "clip_vf must be finite and > 0"),
    (dict(clip_vf=math.inf, values_old=torch.zeros(6)), "clip_vf must be finite and > 0"),
    (dict(clip_vf="0.2", values_old=torch.zeros(6)), "clip_vf must be a Python number"),
    (dict(clip_vf=0.2, values_old=torch.zeros(5)), r"values_old must be a contiguous float32 tensor of shape \(6,\)"),
    (dict(clip_vf=0.2, values_old=torch.zeros(6, dtype=torch.float64)), "values_old must be a contiguous float32"),
    (dict(bounds_coef=-0.1), "bounds_coef must be finite and >= 0"),
    (dict(bounds_coef=math.nan), "bounds_coef must be finite and >= 0"),
    (dict(bounds_coef=True), "bounds_coef must be a Python number"),
    (dict(bounds_coef=0.1), "action_bounds is required with bounds_coef > 0"),
    (dict(bounds_coef=0.1, action_bounds=5), "action_bounds must be a pair"),
    (dict(bounds_coef=0.1, action_bounds=([0.0] * 3, [1.0] * 4)), "action_bounds must be a pair .* of 4 numbers"),
    (dict(bounds_coef=0.1, action_bounds=([0.0, 0.0, math.nan, 0.0], [1.0] * 4)), "must not hold a NaN"),
    (dict(bounds_coef=0.1, action_bounds=([0.0, 2.0, 0.0, 0.0], [1.0] * 4)), "low must be <= high"),
    (dict(action_bounds=([0.0, 2.0, 0.0, 0.0], [1.0] * 4)), "low must be <= high"),  # (checked even where the coefficient is 0)
]


@pytest.mark.parametrize("kw, text", OPTION_REFUSALS)
def test_option_refusals_of_the_python_layer(kw, text):
    eng, a = bare_engine(), _loss_args()
    with pytest.raises(ValueError, match=text):
        eng.ppo_loss(a["mean"], a["log_std"], a["value"], a["actions"], a["logp_old"], a["advantages"], a["returns"], **kw)
    layers = [(torch.zeros(8, 21), torch.zeros(8)), (torch.zeros(4, 8), torch.zeros(4))]
    critic = [(torch.zeros(8, 21), torch.zeros(8)), (torch.zeros(1, 8), torch.zeros(1))]
    with pytest.raises(ValueError, match=text):
        eng.ppo_grad(torch.zeros(6, 21), layers, critic, a["log_std"], a["actions"], a["logp_old"], a["advantages"], a["returns"], **kw)


def test_wrapper_takes_values_old_from_the_batch_dict_only():
    eng, a = bare_engine(), _loss_args()
    batch = dict(actions=a["actions"], logp=a["logp_old"], advantages=a["advantages"], returns=a["returns"])
    with pytest.raises(ValueError, match=r"the batch lacks \['values'\]"):
        pyflyt_amd.ppo_loss(eng, a["mean"], a["log_std"], a["value"], batch, clip_vf=0.2)
    with pytest.raises(ValueError, match="values_old comes from the batch dict"):
        pyflyt_amd.ppo_loss(eng, a["mean"], a["log_std"], a["value"], dict(batch, values=a["value"]), clip_vf=0.2, values_old=a["value"])


def test_adam_argument_rules():
    eng, ok = bare_engine(), [torch.zeros(3, 2), torch.zeros(5)]
    lr = torch.full((1,), 1e-3)
    opt = pyflyt_amd.Adam(eng, ok, lr=lr, target_kl=0.01, kl_stop=1.5, kl_lr=dict(factor=1.5, low=0.5, high=2.0, min=1e-6, max=1e-2))
    assert opt.target_kl == float(torch.tensor(0.01)) and opt.kl_stop == 1.5 and opt.kl_lr["factor"] == 1.5
    assert opt.gate.dtype == torch.int32 and int(opt.gate) == 1 and tuple(opt.kl_state.shape) == (4,) and opt.kl_state.dtype == torch.float64
    plain = pyflyt_amd.Adam(eng, ok)
    assert plain.target_kl is None and set(plain.stats_dict()) == {"step", "grad_norm", "clip_coef", "lr", "skipped"}
    for kw, text in ((dict(target_kl=0.0), "target_kl must be None or a finite Python number > 0"), (dict(target_kl=math.inf), "target_kl"),
                     (dict(target_kl="x"), "target_kl"), (dict(target_kl=0.01, kl_stop=0.5), "kl_stop must be a Python number >= 1"),
                     (dict(target_kl=0.01, kl_stop=math.nan), "kl_stop"), (dict(kl_lr=dict(factor=2.0, low=0.5, high=2.0, min=1e-6, max=1e-2)), "kl_lr comes with target_kl"),
                     (dict(target_kl=0.01, kl_lr=dict(factor=2.0)), "kl_lr must be a dict with the keys"),
                     (dict(target_kl=0.01, kl_lr=dict(factor=1.0, low=0.5, high=2.0, min=1e-6, max=1e-2), lr=lr), "factor > 1"),
                     (dict(target_kl=0.01, kl_lr=dict(factor=2.0, low=2.0, high=2.0, min=1e-6, max=1e-2), lr=lr), "low < high"),
                     (dict(target_kl=0.01, kl_lr=dict(factor=2.0, low=0.5, high=2.0, min=1e-2, max=1e-6), lr=lr), "min <= max"),
                     (dict(target_kl=0.01, kl_lr=dict(factor=2.0, low=0.5, high=2.0, min=0.0, max=1e-2), lr=lr), "finite Python number > 0"),
                     (dict(target_kl=0.01, kl_lr=dict(factor=2.0, low=0.5, high=2.0, min=1e-6, max=1e-2), lr=1e-3), "lr must be a one-element float32 device tensor")):
        with pytest.raises(ValueError, match=text):
            pyflyt_amd.Adam(eng, ok, **kw)
    grads = [torch.zeros(3, 2), torch.zeros(5)]
    with pytest.raises(ValueError, match="stats .* is required with target_kl"):
        opt.step(grads=grads)
    with pytest.raises(ValueError, match="stats is read only with target_kl"):
        plain.step(grads=grads, stats=torch.zeros(16, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"stats must be a contiguous float64 tensor of shape \(16,\)"):
        opt.step(grads=grads, stats=torch.zeros(12, dtype=torch.float64))
    with pytest.raises(ValueError, match="kl_dict\\(\\) needs an optimiser made with target_kl"):
        plain.kl_dict()
    with pytest.raises(ValueError, match=r"gate must be a contiguous .* tensor of shape \(1,\)"):
        eng.kl_control(torch.zeros(16, dtype=torch.float64), torch.zeros(2, dtype=torch.int32), opt.kl_state, 0.01)
    with pytest.raises(ValueError, match="stop_factor must be >= 1"):
        eng.kl_control(torch.zeros(16, dtype=torch.float64), opt.gate, opt.kl_state, 0.01, stop_factor=0.9)
    with pytest.raises(ValueError, match="lr .* is required with adapt"):
        eng.kl_control(torch.zeros(16, dtype=torch.float64), opt.gate, opt.kl_state, 0.01, adapt=True)


def test_state_dict_carries_the_kl_state():
    eng, ok = bare_engine(), [torch.zeros(3, 2), torch.zeros(5)]
    opt = pyflyt_amd.Adam(eng, ok, target_kl=0.01)
    assert set(pyflyt_amd.Adam(eng, ok).state_dict()) == {"state", "param_groups"}
    opt.kl_state.copy_(torch.tensor([0.02, 0.0, 0.0, 3.0], dtype=torch.float64))
    opt.gate.zero_()
    opt.state[5] = 3.0
    sd = opt.state_dict()
    assert sd["kl_control"] == dict(state=[0.02, 0.0, 0.0, 3.0], gate=0, gated_steps=3.0)
    torch.optim.Adam([torch.zeros(3, 2), torch.zeros(5)]).load_state_dict({k: sd[k] for k in ("state", "param_groups")})
    other = pyflyt_amd.Adam(eng, ok, target_kl=0.01)
    other.load_state_dict(sd)
    assert other.kl_state.tolist() == [0.02, 0.0, 0.0, 3.0] and int(other.gate) == 0 and float(other.state[5]) == 3.0
    assert other.kl_dict() == dict(approx_kl=0.02, lr=0.0, gate=0, gated_calls=3, gated_steps=3)
    other.load_state_dict({k: sd[k] for k in ("state", "param_groups")})  # (a checkpoint without it: a fresh control)
    assert other.kl_state.tolist() == [0.0] * 4 and int(other.gate) == 1

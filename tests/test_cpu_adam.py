"""pf_adam_step's host side: the header, the binding, the workspace size (a pure host function, called here without a device), and the
argument checks of the Python layer that need no device."""
import ctypes as C
import os
import re

import pytest
import torch

from bare_engine import bare_engine
import pyflyt_amd
from pyflyt_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pf_sizeof_adam", "pf_adam_workspace_bytes", "pf_adam_step")


def raw_lib():
    if not os.path.exists(L.LIB_PATH):
        pytest.fail(f"{L.LIB_PATH} is not built")
    lib = C.CDLL(L.LIB_PATH)
    lib.pf_sizeof_adam.restype = C.c_size_t
    lib.pf_adam_workspace_bytes.restype = C.c_size_t
    lib.pf_adam_workspace_bytes.argtypes = [C.c_int64]
    return lib


def test_header_declares_the_adam_entry_points():
    text = open(os.path.join(ROOT, "include", "pyflyt_amd.h")).read()
    assert re.search(r"#define\s+PF_ADAM_MAX_TENSORS\s+32\b", text)
    assert re.search(r"typedef\s+struct\s+pf_adam_args\s*\{", text)
    assert re.search(r"size_t\s+pf_sizeof_adam\s*\(\s*void\s*\)", text)
    assert re.search(r"size_t\s+pf_adam_workspace_bytes\s*\(\s*int64_t\s+total_numel\s*\)", text)
    assert re.search(r"int\s+pf_adam_step\s*\(\s*pf_ctx\s*\*\s*\w*\s*,\s*const\s+pf_adam_args\s*\*\s*\w*\s*,\s*void\s*\*\s*workspace\s*,\s*size_t\s+workspace_bytes\s*,"
                     r"\s*void\s*\*\s*stream\s*\)", text)
    assert "fmaf(" in text.split("pf_adam_args")[0].rsplit("The optimiser's step", 1)[1]  # (the float32 sequence is part of the contract)
    for name in NAMES:
        assert name in L.EXPORTS
    assert L.PF_ABI_VERSION == 10 and L.PF_ADAM_MAX_TENSORS == 32


def test_sizeof_adam_matches_the_parsed_mirror():
    assert [f[0] for f in L.PfAdam._fields_] == ["n_tensors", "skip_nonfinite", "lr", "lr_dev", "beta1", "beta2", "eps", "weight_decay", "max_grad_norm",
                                                 "numel", "param", "grad", "exp_avg", "exp_avg_sq", "state"]
    # 2 int32 + lr + padding; the pointer; five floats + padding; 32 x (int64 + four pointers); the state pointer
    assert C.sizeof(L.PfAdam) == 16 + 8 + 24 + 32 * 5 * 8 + 8
    lib = raw_lib()
    assert lib.pf_sizeof_adam() == C.sizeof(L.PfAdam)
    for name in NAMES:
        assert hasattr(lib, name)
    lib.pf_sizeof_mlp.restype = C.c_size_t  # (the existing blocks are as they were)
    assert lib.pf_sizeof_mlp() == C.sizeof(L.PfMlp) == 6 * 4 + 6 * C.sizeof(C.c_void_p)


def test_workspace_bytes_on_the_host():
    """One double per workgroup and a fixed header; the grid is one workgroup per chunk up to a cap, and a chunk holds an element or
    more: positive, non-decreasing in the total, constant above the cap, 0 for a total the call refuses."""
    size = raw_lib().pf_adam_workspace_bytes
    sizes = [size(t) for t in range(1, 4097)]
    assert all(s > 0 and s % 8 == 0 for s in sizes)
    assert all(b >= a for a, b in zip(sizes, sizes[1:]))
    top = sizes[-1]
    header = size(1) - 8
    assert header >= 0
    cap = (top - header) // 8
    assert 1 < cap <= 1024 and sizes[cap - 1] == top and sizes[cap - 2] < top
    for total in (7305, 1 << 20, (1 << 20) + 3, 1 << 30, (1 << 31) - 1):
        assert size(total) == top
    for total in (0, -1, -(1 << 40), 1 << 31, (1 << 31) + 5, 1 << 40):
        assert size(total) == 0


def test_class_refusals_name_the_parameter():
    eng = bare_engine()
    ok = [torch.zeros(3, 2), torch.zeros(5)]
    opt = pyflyt_amd.Adam(eng, ok, lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01, max_grad_norm=0.5)
    assert opt.betas == (float(torch.tensor(0.9)), float(torch.tensor(0.999))) and opt.lr == float(torch.tensor(1e-3))  # (the float32 values)
    assert [tuple(m.shape) for m in opt.exp_avg] == [(3, 2), (5,)] and opt.state.dtype == torch.float64 and tuple(opt.state.shape) == (8,)
    with pytest.raises(ValueError, match="vector env or a BatchEngine"):
        pyflyt_amd.Adam(object(), ok)
    with pytest.raises(ValueError, match=r"params: 1\.\.32 tensors"):
        pyflyt_amd.Adam(eng, [torch.zeros(2) for _ in range(33)])
    with pytest.raises(ValueError, match=r"params: 1\.\.32 tensors"):
        pyflyt_amd.Adam(eng, [])
    with pytest.raises(ValueError, match=r"params\[1\] is the same tensor as params\[0\]"):
        pyflyt_amd.Adam(eng, [ok[0], ok[0]])
    with pytest.raises(ValueError, match=r"params\[1\] must be a contiguous float32"):
        pyflyt_amd.Adam(eng, [ok[0], torch.zeros(4, 3).T])
    with pytest.raises(ValueError, match=r"params\[0\] must be a contiguous float32"):
        pyflyt_amd.Adam(eng, [torch.zeros(4, dtype=torch.float64)])
    with pytest.raises(ValueError, match="there is one group"):
        pyflyt_amd.Adam(eng, [dict(params=ok, lr=1e-3)])
    with pytest.raises(ValueError, match="betas"):
        pyflyt_amd.Adam(eng, ok, betas=(0.9, 1.0))
    with pytest.raises(ValueError, match="eps"):
        pyflyt_amd.Adam(eng, ok, eps=0.0)
    with pytest.raises(ValueError, match="weight_decay"):
        pyflyt_amd.Adam(eng, ok, weight_decay=-1.0)
    with pytest.raises(ValueError, match="lr must be"):
        pyflyt_amd.Adam(eng, ok, lr=float("nan"))
    with pytest.raises(ValueError, match="lr must be"):
        pyflyt_amd.Adam(eng, ok, lr=torch.zeros(2))
    with pytest.raises(ValueError, match="one tensor per parameter"):
        opt.step(grads=[torch.zeros(3, 2)])
    with pytest.raises(ValueError, match=r"grads\[1\] must be a contiguous float32 tensor of shape \(5,\)"):
        opt.step(grads=[torch.zeros(3, 2), torch.zeros(4)])
    opt.step()  # (no parameter has a .grad: nothing to do, nothing called)
    opt.zero_grad()


def test_state_dict_has_torch_layout():
    opt = pyflyt_amd.Adam(bare_engine(), [torch.zeros(3, 2), torch.zeros(5)], lr=1e-3, weight_decay=0.01)
    sd = opt.state_dict()
    assert sd["state"] == {} and sd["param_groups"][0]["params"] == [0, 1]
    ref = torch.optim.AdamW([torch.zeros(3, 2), torch.zeros(5)])
    assert set(ref.state_dict()["param_groups"][0]) == set(sd["param_groups"][0])
    ref.load_state_dict(sd)
    assert ref.param_groups[0]["betas"] == opt.betas and ref.param_groups[0]["lr"] == opt.lr
    opt.state[0] = 4.0
    sd = opt.state_dict()
    assert sorted(sd["state"]) == [0, 1] and float(sd["state"][1]["step"]) == 4.0 and sorted(sd["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
    other = pyflyt_amd.Adam(bare_engine(), [torch.zeros(3, 2), torch.zeros(5)])
    other.load_state_dict(sd)
    assert float(other.state[0]) == 4.0 and other.weight_decay == opt.weight_decay and other.lr == opt.lr
    uneven = opt.state_dict()
    uneven["state"][0]["step"] = torch.tensor(3.0)
    with pytest.raises(ValueError, match="one step counter"):
        other.load_state_dict(uneven)

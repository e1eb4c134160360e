"""pf_ppo_loss's host side: the header / binding, and the argument validation of BatchEngine.ppo_loss that needs no device."""
import ctypes as C
import os
import re

import pytest
import torch

from bare_engine import bare_engine
import pyflyt_amd
from pyflyt_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, A = 12, 4


def test_header_declares_the_ppo_loss_entry_points():
    text = open(os.path.join(ROOT, "include", "pyflyt_amd.h")).read()
    assert re.search(r"typedef\s+struct\s+pf_ppo_loss_args\s*\{", text)
    assert re.search(r"size_t\s+pf_sizeof_ppo_loss\s*\(\s*void\s*\)", text)
    assert re.search(r"int\s+pf_ppo_loss\s*\(\s*pf_ctx\s*\*\s*ctx\s*,\s*const\s+pf_ppo_loss_args\s*\*\s*a\s*,\s*size_t\s+rows\s*,\s*int\s+width\s*,\s*void\s*\*\s*stream\s*\)", text)
    assert "pf_ppo_loss" in L.EXPORTS and "pf_sizeof_ppo_loss" in L.EXPORTS
    assert L.PF_ABI_VERSION == 10


def test_sizeof_ppo_loss_matches_the_parsed_mirror():
    assert [f[0] for f in L.PfPpoLoss._fields_] == ["clip", "vf_coef", "ent_coef", "normalize_advantage", "mean", "log_std", "actions", "logp_old",
                                                    "advantages", "returns", "value", "valid", "grad_mean", "grad_value", "grad_log_std", "stats"]
    assert C.sizeof(L.PfPpoLoss) == 4 * 4 + 12 * C.sizeof(C.c_void_p)
    if not os.path.exists(L.LIB_PATH):
        pytest.fail(f"{L.LIB_PATH} is not built")
    lib = C.CDLL(L.LIB_PATH)
    lib.pf_sizeof_ppo_loss.restype = C.c_size_t
    assert lib.pf_sizeof_ppo_loss() == C.sizeof(L.PfPpoLoss)
    assert hasattr(lib, "pf_ppo_loss")


def test_the_package_exports_the_wrapper():
    assert callable(pyflyt_amd.ppo_loss) and callable(pyflyt_amd.ppo_stats_dict)
    stats = torch.arange(16, dtype=torch.float64)
    d = pyflyt_amd.ppo_stats_dict(stats)
    assert d["valid_rows"] == 0 and d["loss"] == 1.0 and d["approx_kl"] == 5.0 and d["explained_variance"] == 9.0 and d["ratio_max"] == 11.0
    assert len(d) == 12


def good():
    return dict(mean=torch.zeros(M, A), log_std=torch.zeros(A), value=torch.zeros(M), actions=torch.zeros(M, A), logp_old=torch.zeros(M),
                advantages=torch.zeros(M), returns=torch.zeros(M))


@pytest.mark.parametrize("change, fragment", [
    (dict(mean=torch.zeros(M, A, dtype=torch.float64)), "mean must be a contiguous torch.float32"),
    (dict(mean=None), "mean must be a float32 tensor of shape (..., A)"),
    (dict(mean=torch.zeros(M, 9), actions=torch.zeros(M, 9)), "must be in 1..8"),
    (dict(mean=torch.zeros(0, A), actions=torch.zeros(0, A)), "at least one row"),
    (dict(actions=torch.zeros(M, A + 1)), "actions must be a contiguous torch.float32 tensor of shape (12, 4)"),
    (dict(actions=torch.zeros(M + 1, A)), "actions must be a contiguous torch.float32 tensor of shape (12, 4)"),
    (dict(actions=torch.zeros(A, M).T), "actions must be a contiguous"),
    (dict(actions=torch.zeros(M, A, dtype=torch.float16)), "actions must be a contiguous torch.float32"),
    (dict(log_std=torch.zeros(A + 1)), "log_std must be a contiguous torch.float32 tensor of shape (4,)"),
    (dict(value=torch.zeros(M + 1)), "value must be a contiguous torch.float32 tensor of shape (12,)"),
    (dict(value=torch.zeros(M, dtype=torch.float64)), "value must be a contiguous torch.float32"),
    (dict(logp_old=None), "logp_old is required"),
    (dict(advantages=torch.zeros(M, 2)), "advantages must be"),
    (dict(returns=torch.zeros(2 * M)[::2]), "returns must be a contiguous"),
    (dict(valid=torch.zeros(M)), "valid must be a contiguous torch.bool/torch.uint8"),
    (dict(valid=torch.zeros(M - 1, dtype=torch.bool)), "valid must be"),
    (dict(clip=0.0), "clip must be finite and > 0"),
    (dict(clip=-0.2), "clip must be finite and > 0"),
    (dict(clip=float("nan")), "clip must be finite and > 0"),
    (dict(clip=float("inf")), "clip must be finite and > 0"),
    (dict(clip="0.2"), "clip must be a Python number"),
    (dict(clip=torch.tensor(0.2)), "clip must be a Python number"),
    (dict(vf_coef=-1.0), "vf_coef must be finite and >= 0"),
    (dict(vf_coef=True), "vf_coef must be a Python number"),
    (dict(ent_coef=float("nan")), "ent_coef must be finite and >= 0"),
    (dict(ent_coef=None), "ent_coef must be a Python number"),
    (dict(normalize_advantage=1), "normalize_advantage must be a bool"),
    (dict(normalize_advantage="yes"), "normalize_advantage must be a bool"),
])
def test_ppo_loss_refusals_name_the_argument(change, fragment):
    kw = good()
    kw.update(change)
    with pytest.raises(ValueError) as e:
        bare_engine().ppo_loss(**kw)
    assert fragment in str(e.value), str(e.value)


def test_wrapper_refusals():
    eng = bare_engine()
    kw = good()
    with pytest.raises(ValueError, match="vector env or a BatchEngine"):
        pyflyt_amd.ppo_loss(object(), kw["mean"], kw["log_std"], kw["value"], {})
    with pytest.raises(ValueError, match="lacks"):
        pyflyt_amd.ppo_loss(eng, kw["mean"], kw["log_std"], kw["value"], dict(actions=kw["actions"], logp=None, advantages=kw["advantages"], returns=kw["returns"]))
    with pytest.raises(ValueError, match="the four tensors"):
        pyflyt_amd.ppo_loss(eng, kw["mean"], kw["log_std"], kw["value"], kw["actions"], kw["logp_old"])
    with pytest.raises(ValueError, match="clip must be finite"):
        pyflyt_amd.ppo_loss(eng, kw["mean"], kw["log_std"], kw["value"], kw["actions"], kw["logp_old"], kw["advantages"], kw["returns"], clip=0.0)

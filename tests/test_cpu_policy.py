"""pf_rollout_policy's host side: the header / binding, MLPPolicy's validation, the observation-normalisation fold. No GPU."""
import ctypes as C
import os
import re

import pytest
import torch

from pyflyt_amd import MLPPolicy, PyFlytAmdError, build_params
from pyflyt_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _layers(sizes, dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(o, i, generator=g, dtype=dtype) * 0.3, torch.randn(o, generator=g, dtype=dtype) * 0.1) for i, o in zip(sizes[:-1], sizes[1:])]


def test_header_declares_the_policy_entry_points():
    text = open(os.path.join(ROOT, "include", "pyflyt_amd.h")).read()
    assert re.search(r"typedef\s+struct\s+pf_policy\s*\{", text)
    assert re.search(r"size_t\s+pf_sizeof_policy\s*\(\s*void\s*\)", text)
    assert re.search(r"int\s+pf_rollout_policy\s*\(", text)
    assert "pf_sizeof_policy" in L.EXPORTS and "pf_rollout_policy" in L.EXPORTS
    assert L.PF_ABI_VERSION == 10


def test_sizeof_policy_matches_the_parsed_mirror():
    # the mirror: 4 int32, 3 + 3 + 3 pointers (w[3] and b[3] are ARRAYS of pointers)
    assert C.sizeof(L.PfPolicy) == 4 * 4 + 9 * C.sizeof(C.c_void_p)
    assert [f[0] for f in L.PfPolicy._fields_] == ["n_layers", "width", "activation", "w", "b", "log_std", "obs0", "mean_out"]
    if not os.path.exists(L.LIB_PATH):
        pytest.fail(f"{L.LIB_PATH} is not built")
    lib = C.CDLL(L.LIB_PATH)
    lib.pf_sizeof_policy.restype = C.c_size_t
    assert lib.pf_sizeof_policy() == C.sizeof(L.PfPolicy)
    lib.pf_abi_version.restype = C.c_int
    assert lib.pf_abi_version() == 10


@pytest.mark.parametrize("case, field", [("width65", "layers[0].weight"), ("four_layers", "layers"), ("float64", "layers[1].weight"),
                                         ("bias", "layers[0].bias"), ("noncontig", "layers[0].weight")])
def test_mlp_policy_refusals_name_the_field(case, field):
    ls = _layers([21, 64, 64, 4])
    if case == "width65":
        ls = _layers([21, 65, 4])
    elif case == "four_layers":
        ls = _layers([21, 8, 8, 8, 4])
    elif case == "float64":
        ls[1] = (ls[1][0].double(), ls[1][1])
    elif case == "bias":
        ls[0] = (ls[0][0], torch.zeros(63))
    elif case == "noncontig":
        ls[0] = (torch.randn(21, 64).T, ls[0][1])
        assert not ls[0][0].is_contiguous()
    with pytest.raises(ValueError) as e:
        MLPPolicy(ls)
    assert field in str(e.value), str(e.value)


def test_from_torch_round_trips_a_sequential():
    nn = torch.nn
    seq = nn.Sequential(nn.Linear(21, 33), nn.ReLU(), nn.Linear(33, 64), nn.ReLU(), nn.Linear(64, 4))
    pol = MLPPolicy.from_torch(seq, log_std=torch.zeros(4))
    assert pol.activation == "relu" and pol.widths == [33, 64] and pol.obs_dim == 21 and pol.action_dim == 4
    x = torch.randn(50, 21)
    with torch.no_grad():
        assert torch.equal(pol.forward_reference(x, dtype=torch.float32), seq(x))
        # references, not copies: an in-place update of the module is what the policy reads
        seq[0].weight.mul_(0.5)
        assert pol.layers[0][0].data_ptr() == seq[0].weight.data_ptr()
        assert torch.equal(pol.forward_reference(x, dtype=torch.float32), seq(x))
    with pytest.raises(ValueError, match="Tanh or a ReLU"):
        MLPPolicy.from_torch(nn.Sequential(nn.Linear(21, 8), nn.Sigmoid(), nn.Linear(8, 4)))
    with pytest.raises(ValueError, match="Linear"):
        MLPPolicy.from_torch(nn.Sequential(nn.Tanh(), nn.Linear(21, 4), nn.Linear(4, 4)))


def test_observation_normalisation_fold_equals_explicit_normalisation():
    """W' = W / std, b' = b - W' mean, evaluated in fp64. Both sides are the same real number W (x - mean) / std + b; they differ by
    roundings only. Explicit: (x - mean) / std costs 2 roundings per term, the product 1, the D-term sum at most D - 1 more. Folded:
    W / std 1, the product 1, the sum D - 1, and b' itself (a D-term sum with 2 roundings per term, subtracted: D + 2). With
    u = 2^-53 every term of either side is bounded by T = max |W| (|x| + |mean|) / std, so each side is within
    (2 D + 6) u (D T + |b|) of the real value (first order, every rounding counted at the full magnitude of the sum) and the two
    within twice that of each other."""
    torch.manual_seed(3)
    D = 21
    ls = [(w.double(), b.double()) for w, b in _layers([D, 64, 4])]
    mean, std = torch.randn(D, dtype=torch.float64) * 2.0, torch.rand(D, dtype=torch.float64) * 3.0 + 0.1
    x = torch.randn(500, D, dtype=torch.float64) * 3.0
    w, b = ls[0]
    wf = w / std[None, :]
    bf = b - wf @ mean
    folded = x @ wf.T + bf
    explicit = ((x - mean) / std) @ w.T + b
    T = (w.abs().max() * ((x.abs().max() + mean.abs().max()) / std.min())).item()
    bound = 2 * (2 * D + 6) * 2.0 ** -53 * (D * T + b.abs().max().item())
    err = (folded - explicit).abs().max().item()
    print(f"fold error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    # and MLPPolicy's own fold (float32 tensors) is that formula
    ls32 = _layers([D, 64, 4])
    pol = MLPPolicy(ls32, obs_mean=mean.float(), obs_std=std.float())
    wf32 = ls32[0][0] / std.float()[None, :]
    assert torch.equal(pol.device_layers()[0][0], wf32) and torch.equal(pol.device_layers()[0][1], ls32[0][1] - wf32 @ mean.float())
    assert pol.device_layers()[1][0] is ls32[1][0]
    ls32[0][0].mul_(2.0)
    assert not torch.equal(pol.device_layers()[0][0], ls32[0][0] / std.float()[None, :])  # folded layers are copies ...
    pol.refresh()
    assert torch.equal(pol.device_layers()[0][0], ls32[0][0] / std.float()[None, :])  # ... until refresh()


def test_rollout_policy_without_a_device_raises():
    from pyflyt_amd.engine import BatchEngine

    assert hasattr(BatchEngine, "rollout_policy")
    pol = MLPPolicy(_layers([21, 64, 64, 4]))
    if torch.cuda.is_available():  # (with a device there is nothing to refuse: tests/test_gpu_policy_rollout.py runs it)
        return
    with pytest.raises(PyFlytAmdError):
        BatchEngine(build_params("quadx", "hover"), 8).rollout_policy(pol, 4)

"""pf_ppo_grad's host side: the header, the binding, the workspace size (a pure host function, called here without a device), and the
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
NAMES = ("pf_sizeof_ppo_grad", "pf_ppo_grad_workspace_bytes", "pf_ppo_grad")


def raw_lib():
    if not os.path.exists(L.LIB_PATH):
        pytest.fail(f"{L.LIB_PATH} is not built")
    lib = C.CDLL(L.LIB_PATH)
    lib.pf_sizeof_ppo_grad.restype = C.c_size_t
    lib.pf_ppo_grad_workspace_bytes.restype = C.c_size_t
    lib.pf_ppo_grad_workspace_bytes.argtypes = [C.POINTER(L.PfMlp), C.POINTER(L.PfMlp), C.c_int64]
    return lib


def block(in_dim=21, hidden=(64, 64), out_dim=4, activation=0):
    q = L.PfMlp()
    q.n_layers, q.activation, q.in_dim, q.out_dim = len(hidden) + 1, activation, in_dim, out_dim
    for l, w in enumerate(hidden):
        q.width[l] = w
    return q


def n_params(in_dim, hidden, out_dim):
    sizes = [in_dim, *hidden, out_dim]
    return sum(o * i + o for i, o in zip(sizes[:-1], sizes[1:]))


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "pyflyt_amd.h")).read()
    assert re.search(r"typedef\s+struct\s+pf_ppo_grad_args\s*\{", text)
    assert re.search(r"size_t\s+pf_sizeof_ppo_grad\s*\(\s*void\s*\)", text)
    assert re.search(r"size_t\s+pf_ppo_grad_workspace_bytes\s*\(\s*const\s+pf_mlp\s*\*\s*actor\s*,\s*const\s+pf_mlp\s*\*\s*critic\s*,\s*int64_t\s+rows\s*\)", text)
    assert re.search(r"int\s+pf_ppo_grad\s*\(\s*pf_ctx\s*\*\s*ctx\s*,\s*const\s+pf_ppo_grad_args\s*\*\s*a\s*,\s*int64_t\s+rows\s*,\s*void\s*\*\s*workspace\s*,"
                     r"\s*size_t\s+workspace_bytes\s*,\s*void\s*\*\s*stream\s*\)", text)
    for name in NAMES:
        assert name in L.EXPORTS
    assert L.PF_ABI_VERSION == 10


def test_sizeof_matches_the_parsed_mirror():
    assert [f[0] for f in L.PfPpoGradArgs._fields_] == ["clip", "vf_coef", "ent_coef", "normalize_advantage", "actor", "critic", "x", "log_std", "actions",
                                                       "logp_old", "advantages", "returns", "valid", "actor_grad_w", "actor_grad_b", "critic_grad_w",
                                                       "critic_grad_b", "grad_log_std", "stats"]
    assert C.sizeof(L.PfPpoGradArgs) == 4 * 4 + (9 + 12 + 2) * C.sizeof(C.c_void_p)
    lib = raw_lib()
    assert lib.pf_sizeof_ppo_grad() == C.sizeof(L.PfPpoGradArgs)
    for name in NAMES:
        assert hasattr(lib, name)
    # (the existing blocks are as they were)
    lib.pf_sizeof_mlp.restype = lib.pf_sizeof_ppo_loss.restype = C.c_size_t
    assert lib.pf_sizeof_mlp() == C.sizeof(L.PfMlp) == 6 * 4 + 6 * C.sizeof(C.c_void_p)
    assert lib.pf_sizeof_ppo_loss() == C.sizeof(L.PfPpoLoss) == 4 * 4 + 12 * C.sizeof(C.c_void_p)


def test_workspace_bytes_on_the_host():
    """Per workgroup of the tile kernel: a block of float partials per network and one row of twenty doubles. The grid is one
    workgroup per 64-row tile up to a cap: non-decreasing in rows, constant from the cap on."""
    lib = raw_lib()
    for a_shape, c_hidden in (((21, (64, 64), 4), (64,)), ((65, (64, 33), 7), (33, 64)), ((123, (33,), 6), (64,)), ((1, (1,), 1), (1,)), ((128, (64, 64), 8), (64, 64))):
        qa, qc = block(*a_shape), block(a_shape[0], c_hidden, 1)
        per_group = 4 * (n_params(*a_shape) + n_params(a_shape[0], c_hidden, 1)) + 8 * 20
        size = lambda rows: lib.pf_ppo_grad_workspace_bytes(C.byref(qa), C.byref(qc), rows)
        assert size(1) == size(64) == per_group
        assert size(65) == size(128) == 2 * per_group
        sizes = [size(64 * t) for t in range(1, 1025)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:]))
        top = sizes[-1]
        cap = top // per_group
        assert top == cap * per_group and 1 < cap < 1024
        assert sizes[cap - 1] == top and sizes[cap - 2] < top  # (the cap is reached at exactly `cap` tiles)
        for rows in (64 * cap + 1, 1 << 22, (1 << 31) - 65):
            assert size(rows) == top
    # what the call refuses, or no rows: 0
    good_a, good_c = block(), block(hidden=(64,), out_dim=1)
    assert lib.pf_ppo_grad_workspace_bytes(C.byref(good_a), C.byref(good_c), 100) > 0
    for bad_a, bad_c in ((block(hidden=(65, 64)), good_c), (good_a, block(hidden=(65,), out_dim=1)), (block(in_dim=129), block(in_dim=129, hidden=(64,), out_dim=1)),
                         (good_a, block(hidden=(64,), out_dim=2)), (good_a, block(in_dim=22, hidden=(64,), out_dim=1)), (block(out_dim=9), good_c),
                         (block(activation=2), good_c)):
        assert lib.pf_ppo_grad_workspace_bytes(C.byref(bad_a), C.byref(bad_c), 100) == 0
    assert lib.pf_ppo_grad_workspace_bytes(C.byref(good_a), C.byref(good_c), 0) == 0
    assert lib.pf_ppo_grad_workspace_bytes(None, C.byref(good_c), 100) == 0
    assert lib.pf_ppo_grad_workspace_bytes(C.byref(good_a), None, 100) == 0


def layers(in_dim=5, hidden=(6, 7), out_dim=2):
    sizes = [in_dim, *hidden, out_dim]
    return [(torch.zeros(o, i), torch.zeros(o)) for i, o in zip(sizes[:-1], sizes[1:])]


def arguments(**kw):
    a = dict(x=torch.zeros(9, 5), actor=layers(), critic=layers(hidden=(4,), out_dim=1), log_std=torch.zeros(2), actions=torch.zeros(9, 2),
             logp_old=torch.zeros(9), advantages=torch.zeros(9), returns=torch.zeros(9, 1))
    a.update(kw)
    return a


@pytest.mark.parametrize("kw, fragment", [
    (dict(x=torch.zeros(9, 5, dtype=torch.float64)), "x must be a contiguous float32"),
    (dict(x=None), "x must be a float32 tensor of shape (..., in_dim)"),
    (dict(x=torch.zeros(0, 5)), "at least one row"),
    (dict(actor=layers()[:1]), "2 or 3 (weight, bias) pairs"),
    (dict(actor=layers(hidden=(65, 7))), "hidden width 65 is outside 1..64"),
    (dict(actor=layers(out_dim=9), log_std=torch.zeros(9), actions=torch.zeros(9, 9)), "out_dim) must be in 1..8"),
    (dict(critic=layers(in_dim=4, hidden=(4,), out_dim=1)), "layers[0].weight must be a contiguous float32 tensor of shape (4, 5)"),
    (dict(critic=layers(hidden=(4,), out_dim=2)), "the critic's last layer must be 1 wide, got 2"),
    (dict(actor_activation="gelu"), "activation must be 'tanh' or 'relu'"),
    (dict(log_std=torch.zeros(3)), "log_std must be a contiguous torch.float32 tensor of shape (2,)"),
    (dict(log_std=None), "log_std is required"),
    (dict(actions=torch.zeros(9, 3)), "actions must be a contiguous torch.float32 tensor of shape (9, 2)"),
    (dict(actions=torch.zeros(9, 2, dtype=torch.float64)), "actions must be a contiguous torch.float32"),
    (dict(logp_old=torch.zeros(8)), "logp_old must be a contiguous torch.float32 tensor of shape (9,)"),
    (dict(advantages=None), "advantages is required"),
    (dict(returns=torch.zeros(9, 2)), "returns must be a contiguous torch.float32 tensor of shape (9,)"),
    (dict(valid=torch.zeros(9)), "valid must be a contiguous torch.bool/torch.uint8 tensor of shape (9,)"),
    (dict(clip=0.0), "clip must be finite and > 0"),
    (dict(clip="0.2"), "clip must be a Python number"),
    (dict(vf_coef=-1.0), "vf_coef must be finite and >= 0"),
    (dict(ent_coef=float("nan")), "ent_coef must be finite and >= 0"),
    (dict(normalize_advantage=1), "normalize_advantage must be a bool"),
])
def test_engine_refusals_name_the_argument(kw, fragment):
    with pytest.raises(ValueError) as e:
        bare_engine().ppo_grad(**arguments(**kw))  # (an engine without a context or a library: a refusal comes before either is touched)
    assert fragment in str(e.value), str(e.value)


def test_wrapper_is_exported_and_refuses():
    nn = torch.nn
    assert pyflyt_amd.ppo_grad is pyflyt_amd.ppo.ppo_grad and "ppo_grad" in pyflyt_amd.__all__
    eng, x = bare_engine(), torch.zeros(9, 5)
    actor, critic = nn.Sequential(nn.Linear(5, 6), nn.Tanh(), nn.Linear(6, 2)), nn.Sequential(nn.Linear(5, 4), nn.Tanh(), nn.Linear(4, 1))
    log_std = nn.Parameter(torch.zeros(2))
    batch = (torch.zeros(9, 2), torch.zeros(9), torch.zeros(9), torch.zeros(9))
    with pytest.raises(ValueError, match="vector env or a BatchEngine"):
        pyflyt_amd.ppo_grad(object(), x, actor, critic, log_std, *batch)
    with pytest.raises(ValueError, match="produces no gradient for x"):
        pyflyt_amd.ppo_grad(eng, torch.zeros(9, 5, requires_grad=True), actor, critic, log_std, *batch)
    with pytest.raises(ValueError, match="actor: the Sequential must end with a Linear"):
        pyflyt_amd.ppo_grad(eng, x, nn.Sequential(nn.Linear(5, 6), nn.Tanh()), critic, log_std, *batch)
    with pytest.raises(ValueError, match="critic: module 1 must be a Tanh or a ReLU"):
        pyflyt_amd.ppo_grad(eng, x, actor, nn.Sequential(nn.Linear(5, 4), nn.Sigmoid(), nn.Linear(4, 1)), log_std, *batch)
    with pytest.raises(ValueError, match="comes with activation"):
        pyflyt_amd.ppo_grad(eng, x, layers(), critic, log_std, *batch)
    with pytest.raises(ValueError, match="critic must be a torch.nn.Sequential or a list"):
        pyflyt_amd.ppo_grad(eng, x, actor, 3, log_std, *batch)
    with pytest.raises(ValueError, match="give the dict env.collect returned, or the four tensors"):
        pyflyt_amd.ppo_grad(eng, x, actor, critic, log_std, *batch[:3])
    with pytest.raises(ValueError, match="the batch lacks"):
        pyflyt_amd.ppo_grad(eng, x, actor, critic, log_std, dict(actions=batch[0], advantages=batch[2], returns=batch[3]))
    with pytest.raises(ValueError, match="valid comes from the batch dict"):
        pyflyt_amd.ppo_grad(eng, x, actor, critic, log_std, dict(actions=batch[0], logp=batch[1], advantages=batch[2], returns=batch[3]), valid=torch.ones(9, dtype=torch.bool))
    with pytest.raises(ValueError, match="log_std must be a float32 tensor"):
        pyflyt_amd.ppo_grad(eng, x, actor, critic, None, *batch)
    with pytest.raises(ValueError, match="clip must be finite and > 0"):
        pyflyt_amd.ppo_grad(eng, x, actor, critic, log_std, *batch, clip=-0.2)
    assert all(p.grad is None for p in list(actor.parameters()) + list(critic.parameters()) + [log_std])

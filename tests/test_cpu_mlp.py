"""pf_mlp_forward / pf_mlp_backward's host side: the header, the binding, the workspace size (a pure host function, called here
without a device), and the argument checks of the Python layer that need no device."""
import ctypes as C
import os
import re

import pytest
import torch

from bare_engine import bare_engine
import pyflyt_amd
from pyflyt_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pf_sizeof_mlp", "pf_mlp_forward", "pf_mlp_backward_workspace_bytes", "pf_mlp_backward")


def raw_lib():
    if not os.path.exists(L.LIB_PATH):
        pytest.fail(f"{L.LIB_PATH} is not built")
    lib = C.CDLL(L.LIB_PATH)
    lib.pf_sizeof_mlp.restype = C.c_size_t
    lib.pf_mlp_backward_workspace_bytes.restype = C.c_size_t
    lib.pf_mlp_backward_workspace_bytes.argtypes = [C.POINTER(L.PfMlp), C.c_int64]
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


def test_header_declares_the_mlp_entry_points():
    text = open(os.path.join(ROOT, "include", "pyflyt_amd.h")).read()
    assert re.search(r"typedef\s+struct\s+pf_mlp\s*\{", text)
    assert re.search(r"size_t\s+pf_sizeof_mlp\s*\(\s*void\s*\)", text)
    assert re.search(r"int\s+pf_mlp_forward\s*\(\s*pf_ctx\s*\*\s*\w*\s*,\s*const\s+pf_mlp\s*\*\s*\w*\s*,\s*const\s+float\s*\*\s*x\s*,\s*int64_t\s+rows\s*,"
                     r"\s*float\s*\*\s*out\s*,\s*void\s*\*\s*stream\s*\)", text)
    assert re.search(r"size_t\s+pf_mlp_backward_workspace_bytes\s*\(\s*const\s+pf_mlp\s*\*\s*\w*\s*,\s*int64_t\s+rows\s*\)", text)
    assert re.search(r"int\s+pf_mlp_backward\s*\(\s*pf_ctx\s*\*\s*\w*\s*,\s*const\s+pf_mlp\s*\*\s*\w*\s*,\s*const\s+float\s*\*\s*x\s*,\s*const\s+float\s*\*\s*grad_out\s*,"
                     r"\s*int64_t\s+rows\s*,\s*float\s*\*\s*const\s+grad_w\s*\[\s*3\s*\]\s*,\s*float\s*\*\s*const\s+grad_b\s*\[\s*3\s*\]\s*,\s*void\s*\*\s*workspace\s*,"
                     r"\s*size_t\s+workspace_bytes\s*,\s*void\s*\*\s*stream\s*\)", text)
    assert "non-finite" in text or "NaN or an infinity in x poisons" in text  # (the zero-gradient caveat is part of the contract)
    for name in NAMES:
        assert name in L.EXPORTS
    assert L.PF_ABI_VERSION == 10


def test_sizeof_mlp_matches_the_parsed_mirror():
    assert [f[0] for f in L.PfMlp._fields_] == ["n_layers", "width", "activation", "in_dim", "out_dim", "w", "b"]
    assert C.sizeof(L.PfMlp) == 6 * 4 + 6 * C.sizeof(C.c_void_p)
    lib = raw_lib()
    assert lib.pf_sizeof_mlp() == C.sizeof(L.PfMlp)
    for name in NAMES:
        assert hasattr(lib, name)
    # (the existing block is as it was)
    lib.pf_sizeof_policy.restype = C.c_size_t
    assert lib.pf_sizeof_policy() == C.sizeof(L.PfPolicy) == 4 * 4 + 9 * C.sizeof(C.c_void_p)


def test_workspace_bytes_on_the_host():
    """One block of partial sums -- a float per parameter -- for every workgroup; the grid is one workgroup per 64-row tile up to a
    cap: monotone in rows up to it, constant above it."""
    lib = raw_lib()
    for shape in ((21, (64, 64), 4), (21, (64,), 1), (123, (33, 64), 6), (1, (1,), 1), (128, (64, 64), 8)):
        q, P = block(*shape), n_params(*shape)
        size = lambda rows: lib.pf_mlp_backward_workspace_bytes(C.byref(q), rows)
        assert size(1) == size(64) == 4 * P
        assert size(65) == size(128) == 2 * 4 * P
        sizes = [size(64 * t) for t in range(1, 2049)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:]))
        top = sizes[-1]
        cap = top // (4 * P)
        assert top == cap * 4 * P and 1 < cap < 2048
        assert sizes[cap - 1] == top and sizes[cap - 2] < top  # (the cap is reached at exactly `cap` tiles)
        for rows in (64 * cap + 1, 1 << 22, (1 << 31) - 65):
            assert size(rows) == top
    # a shape the calls refuse, or no rows: 0
    for bad in (block(in_dim=0), block(in_dim=129), block(out_dim=0), block(out_dim=9), block(hidden=(65, 64)), block(hidden=(64, 0)), block(activation=2)):
        assert lib.pf_mlp_backward_workspace_bytes(C.byref(bad), 100) == 0
    bad = block()
    bad.n_layers = 4
    assert lib.pf_mlp_backward_workspace_bytes(C.byref(bad), 100) == 0
    assert lib.pf_mlp_backward_workspace_bytes(C.byref(block()), 0) == 0
    assert lib.pf_mlp_backward_workspace_bytes(None, 100) == 0


def layers(in_dim=5, hidden=(6, 7), out_dim=2):
    sizes = [in_dim, *hidden, out_dim]
    return [(torch.zeros(o, i), torch.zeros(o)) for i, o in zip(sizes[:-1], sizes[1:])]


@pytest.mark.parametrize("kw, fragment", [
    (dict(x=torch.zeros(9, 5, dtype=torch.float64)), "x must be a contiguous float32"),
    (dict(x=torch.zeros(5, 9).T), "x must be a contiguous float32"),
    (dict(x=torch.zeros(9, 4)), "layers[0].weight must be a contiguous float32 tensor of shape (6, 4)"),
    (dict(x=torch.zeros(0, 5)), "at least one row"),
    (dict(x=None), "x must be a float32 tensor of shape (..., in_dim)"),
    (dict(activation="gelu"), "activation must be 'tanh' or 'relu'"),
    (dict(layers=layers()[:1]), "2 or 3 (weight, bias) pairs"),
    (dict(layers=layers(hidden=(65, 7))), "hidden width 65 is outside 1..64"),
    (dict(layers=layers(out_dim=9)), "out_dim) must be in 1..8"),
    (dict(x=torch.zeros(9, 129), layers=layers(in_dim=129)), "in_dim) must be in 1..128"),
    (dict(layers=[layers()[0], (torch.zeros(7, 5), torch.zeros(7)), layers()[2]]), "layers[1].weight must be a contiguous float32 tensor of shape (7, 6)"),
    (dict(layers=[layers()[0], (torch.zeros(7, 6), torch.zeros(6)), layers()[2]]), "layers[1].bias must be a contiguous float32 tensor of shape (7,)"),
    (dict(layers=[(torch.zeros(6, 5, dtype=torch.float16), torch.zeros(6)), *layers()[1:]]), "layers[0].weight must be a contiguous float32"),
    (dict(out=torch.zeros(9, 3)), "out must be a contiguous float32 tensor of shape (9, 2)"),
    (dict(grad_out=torch.zeros(9, 3)), "grad_out must be a contiguous float32 tensor of shape (9, 2)"),
    (dict(grad_out=torch.zeros(9, 2, dtype=torch.float64)), "grad_out must be a contiguous float32"),
    (dict(grad_out=None), "grad_out must be a float32 tensor of shape (9, 2)"),
])
def test_engine_refusals_name_the_argument(kw, fragment):
    a = dict(x=torch.zeros(9, 5), layers=layers(), activation="tanh")
    backward = "grad_out" in kw
    a.update(kw)
    with pytest.raises(ValueError) as e:
        if backward:
            bare_engine().mlp_backward(a["x"], a["grad_out"], a["layers"], a["activation"])
        else:
            bare_engine().mlp_forward(a["x"], a["layers"], a["activation"], out=a.get("out"))
    assert fragment in str(e.value), str(e.value)


def test_wrapper_refusals():
    nn = torch.nn
    eng, x = bare_engine(), torch.zeros(9, 5)
    seq = nn.Sequential(nn.Linear(5, 6), nn.Tanh(), nn.Linear(6, 2))
    assert callable(pyflyt_amd.mlp)
    with pytest.raises(ValueError, match="vector env or a BatchEngine"):
        pyflyt_amd.mlp(object(), x, seq)
    with pytest.raises(ValueError, match="produces no gradient for x"):
        pyflyt_amd.mlp(eng, torch.zeros(9, 5, requires_grad=True), seq)
    with pytest.raises(ValueError, match="must end with a Linear"):
        pyflyt_amd.mlp(eng, x, nn.Sequential(nn.Linear(5, 6), nn.Tanh()))
    with pytest.raises(ValueError, match="must be a Tanh or a ReLU"):
        pyflyt_amd.mlp(eng, x, nn.Sequential(nn.Linear(5, 6), nn.Sigmoid(), nn.Linear(6, 2)))
    with pytest.raises(ValueError, match="one kind of activation"):
        pyflyt_amd.mlp(eng, x, nn.Sequential(nn.Linear(5, 6), nn.Tanh(), nn.Linear(6, 6), nn.ReLU(), nn.Linear(6, 2)))
    with pytest.raises(ValueError, match="Linear with a bias"):
        pyflyt_amd.mlp(eng, x, nn.Sequential(nn.Linear(5, 6, bias=False), nn.Tanh(), nn.Linear(6, 2)))
    with pytest.raises(ValueError, match="comes with activation"):
        pyflyt_amd.mlp(eng, x, layers())
    with pytest.raises(ValueError, match="Sequential or a list"):
        pyflyt_amd.mlp(eng, x, 3)

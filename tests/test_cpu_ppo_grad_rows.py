"""The host side of pf_ppo_grad_rows (minibatches by an index list): the header's text, the binding, the refusals of the C function that
need no device (a NULL ctx, bad scalars), pyflyt_amd.minibatches on the CPU and the rows= checks of the Python layer."""
import ctypes as C
import os
import re

import pytest
import torch

from bare_engine import bare_engine
import pyflyt_amd
from pyflyt_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = (1 << 31) - 64


def test_header_states_the_contract():
    text = open(os.path.join(ROOT, "include", "pyflyt_amd.h")).read()
    bare = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    assert re.search(r"int\s+pf_ppo_grad_rows\s*\(\s*pf_ctx\s*\*\s*\w+,\s*const\s+pf_ppo_grad_args\s*\*\s*\w+,\s*const\s+pf_ppo_options\s*\*\s*\w+\s*,"
                     r"\s*const\s+int32_t\s*\*\s*row_index\s*,\s*int64_t\s+m,\s*int64_t\s+rows_total,\s*void\s*\*\s*workspace,\s*size_t\s+workspace_bytes,"
                     r"\s*void\s*\*\s*stream\s*\)", bare)
    contract = text.split("int pf_ppo_grad_rows")[0].rsplit("A minibatch of a PPO epoch", 1)[1]
    for fragment in ("t'[j] = t[row_index[j]]", "BIT IDENTITY", "PER MINIBATCH", "Duplicates are allowed", "OUT OF RANGE", "never dereferenced", "stats[14]",
                     "row 0", "pf_ppo_grad_workspace_bytes(actor, critic, m)", "rows_total rows, not m", "values_old"):
        assert fragment in contract, fragment
    assert "#define PF_ABI_VERSION 10" in text and L.PF_ABI_VERSION == 10
    assert "pf_ppo_grad_rows" in L.EXPORTS
    # (every existing block is as it was: the sizes the library reports are checked against the header's at load, in L.lib())


def test_binding():
    if not os.path.exists(L.LIB_PATH):
        pytest.fail(f"{L.LIB_PATH} is not built")
    lib = L.lib()
    assert hasattr(C.CDLL(L.LIB_PATH), "pf_ppo_grad_rows")
    want = [C.c_void_p, C.POINTER(L.PfPpoGradArgs), C.POINTER(L.PfPpoOptions), C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]
    assert list(lib.pf_ppo_grad_rows.argtypes) == want
    assert lib.pf_abi_version() == 10


def test_c_function_refuses_bad_scalars_and_a_null_ctx():
    lib = L.lib()
    err = lambda: lib.pf_last_error(None).decode()  # noqa: E731
    g, o = L.PfPpoGradArgs(), L.PfPpoOptions()
    idx = (C.c_int32 * 4)(0, 1, 2, 3)  # (never read: every call here is refused on the host)
    p = C.cast(idx, C.c_void_p)
    who = "pf_ppo_grad_rows: "
    for m, total, index, text in ((0, 8, p, "m must be >= 1"), (-4, 8, p, "m must be >= 1"), (BIG, 8, p, "m must be below 2^31 - 64"),
                                  (4, 0, p, "rows_total must be >= 1"), (4, -1, p, "rows_total must be >= 1"),
                                  (4, BIG, p, "rows_total must be below 2^31 - 64"), (4, 8, None, "row_index is required"),
                                  (4, 8, p, "ctx is required"), (BIG - 1, BIG - 1, p, "ctx is required")):
        for options in (None, C.byref(o)):
            assert lib.pf_ppo_grad_rows(None, C.byref(g), options, index, m, total, None, 0, None) == L.ERR_ARG
            assert err().startswith(who + text), err()
    assert lib.pf_ppo_grad_opt(None, C.byref(g), None, 8, None, 0, None) == L.ERR_ARG and err() == "pf_ppo_grad_opt: ctx is required"  # (as it was)


def test_minibatches_on_the_cpu():
    for M, k in ((10, 3), (4096, 4), (7, 7), (1000, 32), (5, 1)):
        g = torch.Generator().manual_seed(5)
        parts = pyflyt_amd.minibatches(M, k, device="cpu", generator=g)
        assert len(parts) == k and all(p.dtype == torch.int32 and p.dim() == 1 and p.is_contiguous() and p.device.type == "cpu" for p in parts)
        sizes = [p.numel() for p in parts]
        assert sum(sizes) == M and max(sizes) - min(sizes) <= 1 and min(sizes) >= 1
        assert sorted(torch.cat(parts).tolist()) == list(range(M))
        base = parts[0].untyped_storage().data_ptr()
        assert all(p.untyped_storage().data_ptr() == base for p in parts)  # views of ONE permutation: nothing was copied
        again = pyflyt_amd.minibatches(M, k, device="cpu", generator=torch.Generator().manual_seed(5))
        assert all(torch.equal(u, v) for u, v in zip(parts, again))
    a = pyflyt_amd.minibatches(4096, 4, device="cpu", generator=torch.Generator().manual_seed(1))
    b = pyflyt_amd.minibatches(4096, 4, device="cpu", generator=torch.Generator().manual_seed(2))
    assert not torch.equal(torch.cat(a), torch.cat(b)) and not torch.equal(torch.cat(a), torch.arange(4096, dtype=torch.int32))
    assert "minibatches" in pyflyt_amd.__all__
    for args, text in (((0, 1), "total_rows must be an int >= 1"), ((8, 0), "n_minibatches must be an int >= 1"), ((8.0, 2), "total_rows must be an int"),
                       ((8, True), "n_minibatches must be an int"), ((4, 5), "n_minibatches must be at most total_rows"), ((BIG, 2), "below 2\\^31 - 64")):
        with pytest.raises(ValueError, match=text):
            pyflyt_amd.minibatches(*args, device="cpu")


def test_stats_dict_names_slot_14():
    stats = torch.arange(16, dtype=torch.float64)
    d = pyflyt_amd.ppo_stats_dict(stats, options=True, rows=True)
    assert d["index_out_of_range"] == 14 and isinstance(d["index_out_of_range"], int) and d["bounds_loss"] == 13.0 and len(d) == 15
    assert pyflyt_amd.ppo_stats_dict(stats, rows=True)["index_out_of_range"] == 14 and len(pyflyt_amd.ppo_stats_dict(stats, rows=True)) == 13
    assert "index_out_of_range" not in pyflyt_amd.ppo_stats_dict(stats, options=True)  # (without rows=True the dict is what it was)


ROWS_REFUSALS = [
    ([0, 1, 2], "rows must be a 1-D int32 tensor of row numbers, got list"),
    (3, "rows must be a 1-D int32 tensor of row numbers, got int"),
    (torch.zeros(2, 3, dtype=torch.int32), r"rows must be a 1-D int32 tensor of row numbers, got \(2, 3\)"),
    (torch.zeros((), dtype=torch.int32), r"rows must be a 1-D int32 tensor of row numbers, got \(\)"),
    (torch.zeros(0, dtype=torch.int32), "rows must name at least one row"),
    (torch.zeros(4, dtype=torch.int64), r"rows must be a contiguous int32 tensor of shape \(4,\) on cpu, got torch.int64"),
    (torch.zeros(4, dtype=torch.float32), r"rows must be a contiguous int32 tensor of shape \(4,\) on cpu, got torch.float32"),
    (torch.zeros(8, dtype=torch.int32)[::2], r"rows must be a contiguous int32 tensor of shape \(4,\)"),
]


@pytest.mark.parametrize("rows, text", ROWS_REFUSALS)
def test_rows_refusals_of_the_python_layer(rows, text):
    eng, M, A = bare_engine(), 6, 4
    actor = [(torch.zeros(8, 21), torch.zeros(8)), (torch.zeros(A, 8), torch.zeros(A))]
    critic = [(torch.zeros(8, 21), torch.zeros(8)), (torch.zeros(1, 8), torch.zeros(1))]
    batch = (torch.zeros(M, A), torch.zeros(M), torch.zeros(M), torch.zeros(M))
    with pytest.raises(ValueError, match=text):
        eng.ppo_grad(torch.zeros(M, 21), actor, critic, torch.zeros(A), *batch, rows=rows)
    with pytest.raises(ValueError, match=text):
        pyflyt_amd.ppo_grad(eng, torch.zeros(M, 21), actor, critic, torch.zeros(A), *batch, activation="tanh", rows=rows)

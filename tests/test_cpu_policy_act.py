"""pf_policy_act's surface without a GPU: the header's prototype, the export list, the binding's argument types, pf_policy as it was."""
import ctypes as C
import re

from pyflyt_amd import _lib as L


def test_header_declares_the_prototype():
    text = " ".join(open(L.HEADER_PATH).read().split())
    assert "int pf_policy_act(pf_ctx* ctx, const pf_policy* policy, float* actions_out, uint32_t step_index, void* stream);" in text
    assert re.search(r"#define\s+PF_ABI_VERSION\s+10\b", text)  # (a new function only)


def test_exported():
    assert "pf_policy_act" in L.EXPORTS


def test_binding_has_its_argtypes():
    lib = L.lib()  # (loads the library: every name of EXPORTS must be there, every struct size must match)
    assert lib.pf_policy_act.argtypes == [C.c_void_p, C.POINTER(L.PfPolicy), C.c_void_p, C.c_uint32, C.c_void_p]


def test_pf_policy_is_unchanged():
    # n_layers, width[2], activation (16 bytes), w[3], b[3], log_std, obs0, mean_out (nine pointers)
    assert C.sizeof(L.PfPolicy) == 16 + 9 * C.sizeof(C.c_void_p) == 88
    assert [name for name, _ in L.PfPolicy._fields_] == ["n_layers", "width", "activation", "w", "b", "log_std", "obs0", "mean_out"]
    assert L.lib().pf_sizeof_policy() == C.sizeof(L.PfPolicy)

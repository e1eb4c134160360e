"""pf_world_sync's surface without a GPU: the header's declarations, the export list, the struct mirror, and what
BatchEngine.rollout_policy_worlds refuses before any launch -- on an engine made without __init__ (tests/bare_engine.py)."""
import ctypes as C
import re

import pytest
import torch

from bare_engine import N, bare_engine
from pyflyt_amd import _lib as L
from pyflyt_amd import build_params


def test_header_declares_the_struct_and_the_prototypes():
    text = " ".join(open(L.HEADER_PATH).read().split())
    assert "typedef struct pf_world_sync_args {" in text and "} pf_world_sync_args;" in text
    assert "size_t pf_sizeof_world_sync(void);" in text
    assert "int pf_world_sync(pf_ctx* ctx, const pf_world_sync_args* a, int agents_per_world, void* stream);" in text
    assert re.search(r"#define\s+PF_ABI_VERSION\s+10\b", text)  # (a new function only)
    assert L.PF_ABI_VERSION == 10


def test_exported():
    assert "pf_world_sync" in L.EXPORTS and "pf_sizeof_world_sync" in L.EXPORTS


def test_struct_mirror():
    assert [name for name, _ in L.PfWorldSync._fields_] == ["terminated", "truncated", "reward", "done", "exclude", "valid_out", "reset_out"]
    assert C.sizeof(L.PfWorldSync) == 7 * C.sizeof(C.c_void_p)
    lib = L.lib()  # (loads the library: every name of EXPORTS must be there, every struct size must match)
    assert lib.pf_sizeof_world_sync() == C.sizeof(L.PfWorldSync)
    assert lib.pf_world_sync.argtypes == [C.c_void_p, C.POINTER(L.PfWorldSync), C.c_int, C.c_void_p]


def _off_engine():
    return bare_engine(autoreset="off")


def test_refuses_an_engine_without_an_env_task():
    eng = _off_engine()
    eng.params = build_params("quadx", "none")
    with pytest.raises(ValueError, match="needs an engine with an env task"):
        eng.rollout_policy_worlds(None, 4, 4)


def test_refuses_an_auto_reset_mode_and_points_at_the_stepwise_rollout():
    for mode in ("next_step", "same_step"):
        with pytest.raises(ValueError, match="auto-reset OFF.*rollout_policy_steps"):
            bare_engine(autoreset=mode).rollout_policy_worlds(None, 4, 4)


def test_refuses_injected_noise():
    eng = _off_engine()
    eng.params = build_params("quadx", "hover", autoreset="off", noise="inject")
    with pytest.raises(ValueError, match="PF_NOISE_INJECT"):
        eng.rollout_policy_worlds(None, 4, 4)


@pytest.mark.parametrize("k", [0, -3])
def test_refuses_no_steps(k):
    with pytest.raises(ValueError, match="k_steps must be >= 1"):
        _off_engine().rollout_policy_worlds(None, k, 4)


@pytest.mark.parametrize("apw", [0, -1, 65, 3, 5])  # (N = 8 lanes: 3 and 5 do not divide them)
def test_refuses_worlds_that_do_not_tile_the_lanes(apw):
    assert N == 8
    with pytest.raises(ValueError, match="agents_per_world must be in 1..64 and divide the lane count 8"):
        _off_engine().rollout_policy_worlds(None, 4, apw)
    with pytest.raises(ValueError, match="agents_per_world must be in 1..64 and divide the lane count 8"):
        _off_engine().world_sync(None, None, None, None, apw)


def test_refuses_half_an_opponent():
    lanes = torch.zeros(N, dtype=torch.bool)
    with pytest.raises(ValueError, match="opponent and opponent_lanes come together"):
        _off_engine().rollout_policy_worlds(None, 4, 4, opponent=object())
    with pytest.raises(ValueError, match="opponent and opponent_lanes come together"):
        _off_engine().rollout_policy_worlds(None, 4, 4, opponent_lanes=lanes)


def test_the_policy_is_checked_behind_the_refusals_and_before_any_tensor():
    with pytest.raises(ValueError, match="policy must be a pyflyt_amd.MLPPolicy"):
        _off_engine().rollout_policy_worlds(None, 4, 4)
    with pytest.raises(ValueError, match="policy must be a pyflyt_amd.MLPPolicy"):
        _off_engine().collect_rollout_worlds("not a policy", 4, 2)


def test_world_sync_checks_its_tensors():
    eng = _off_engine()
    flags, reward = torch.zeros(N, dtype=torch.bool), torch.zeros(N)
    with pytest.raises(ValueError, match="terminated is required"):
        eng.world_sync(None, flags, reward, flags, 4)
    with pytest.raises(ValueError, match=r"reward must be a contiguous float32 tensor of shape \(8,\)"):
        eng.world_sync(flags, flags, reward.double(), flags, 4)
    with pytest.raises(ValueError, match=r"done must be a contiguous torch.bool/torch.uint8 tensor of shape \(8,\)"):
        eng.world_sync(flags, flags, reward, torch.zeros(N + 1, dtype=torch.uint8), 4)
    with pytest.raises(ValueError, match=r"exclude must be a contiguous torch.bool/torch.uint8 tensor"):
        eng.world_sync(flags, flags, reward, flags, 4, exclude=reward)

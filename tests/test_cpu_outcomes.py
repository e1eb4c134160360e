"""pf_episode_outcomes' surface without a GPU: the header's constants and declarations, the export list, the struct mirror, and what
BatchEngine.episode_outcomes and the closed loops with outcomes=True refuse before any launch -- on an engine made without __init__
(tests/bare_engine.py)."""
import ctypes as C
import re

import pytest
import torch

from bare_engine import N, bare_engine
from pyflyt_amd import _lib as L
from pyflyt_amd import MLPPolicy, build_params


def test_header_declares_the_constants_the_struct_and_the_prototypes():
    text = " ".join(open(L.HEADER_PATH).read().split())
    assert "typedef struct pf_outcome_args {" in text and "} pf_outcome_args;" in text
    assert "size_t pf_sizeof_outcome(void);" in text
    assert "int pf_episode_outcomes(pf_ctx* ctx, const pf_outcome_args* a, int k_steps, int agents_per_world, void* stream);" in text
    assert re.search(r"#define\s+PF_OUTCOME_SLOTS\s+16\b", text) and re.search(r"#define\s+PF_OUTCOME_MAX_GROUPS\s+16\b", text)
    assert re.search(r"#define\s+PF_ABI_VERSION\s+10\b", text)  # (a new function only)
    assert L.PF_ABI_VERSION == 10 and L.PF_OUTCOME_SLOTS == 16 and L.PF_OUTCOME_MAX_GROUPS == 16


def test_outcome_bits():
    bits = [L.PF_OC_ENDED, L.PF_OC_TERMINATED, L.PF_OC_COLLISION, L.PF_OC_OOB, L.PF_OC_COMPLETE, L.PF_OC_DEAD, L.PF_OC_NONFINITE]
    assert bits == [1, 2, 4, 8, 16, 32, 64]  # (a byte holds them all)
    assert len(L.OUTCOME_SLOT_NAMES) == 14 and L.OUTCOME_SLOT_NAMES[0] == "episodes" and L.OUTCOME_SLOT_NAMES[10] == "worlds"


def test_exported():
    assert "pf_episode_outcomes" in L.EXPORTS and "pf_sizeof_outcome" in L.EXPORTS


def test_struct_mirror():
    assert [name for name, _ in L.PfOutcome._fields_] == ["terminated", "truncated", "valid", "info", "state", "group", "n_groups", "world_reset",
                                                          "world_latch", "outcome_out", "counts"]
    assert C.sizeof(L.PfOutcome) == 11 * C.sizeof(C.c_void_p)  # (n_groups is padded to the pointers' alignment)
    lib = L.lib()  # (loads the library: every name of EXPORTS must be there, every struct size must match)
    assert lib.pf_sizeof_outcome() == C.sizeof(L.PfOutcome)
    assert lib.pf_episode_outcomes.argtypes == [C.c_void_p, C.POINTER(L.PfOutcome), C.c_int, C.c_int, C.c_void_p]


def test_the_library_refuses_a_null_context_and_block():
    lib = L.lib()
    assert lib.pf_episode_outcomes(None, C.byref(L.PfOutcome()), 1, 1, None) == L.ERR_ARG
    assert b"pf_episode_outcomes" in lib.pf_last_error(None) and b"ctx" in lib.pf_last_error(None)


def _flags(k=None):
    return torch.zeros(N, dtype=torch.bool) if k is None else torch.zeros(k, N, dtype=torch.bool)


def _counts(g=1):
    return torch.zeros(g, 16, dtype=torch.int64)


def test_refuses_an_engine_without_an_env_task():
    eng = bare_engine()
    eng.params = build_params("quadx", "none")
    with pytest.raises(ValueError, match="needs an engine with an env task"):
        eng.episode_outcomes(_flags(), _flags(), _counts())


def test_refuses_no_flags_and_no_steps():
    with pytest.raises(ValueError, match="terminated is required"):
        bare_engine().episode_outcomes(None, _flags(), _counts())
    with pytest.raises(ValueError, match="at least one step"):
        bare_engine().episode_outcomes(_flags(0), _flags(0), _counts())
    with pytest.raises(ValueError, match="truncated is required"):
        bare_engine().episode_outcomes(_flags(), None, _counts())
    with pytest.raises(ValueError, match="counts is required"):
        bare_engine().episode_outcomes(_flags(), _flags(), None)


def test_refuses_a_trajectory_without_info():
    with pytest.raises(ValueError, match="info is required for a trajectory of k > 1 steps"):
        bare_engine().episode_outcomes(_flags(3), _flags(3), _counts())


@pytest.mark.parametrize("g", [0, 17, -1, 2.0, True])
def test_refuses_group_counts_outside_the_block(g):
    with pytest.raises(ValueError, match=r"n_groups must be an int in 1..16"):
        bare_engine().episode_outcomes(_flags(), _flags(), _counts(), n_groups=g)


@pytest.mark.parametrize("apw", [0, -1, 65, 3, 5])  # (N = 8 lanes: 3 and 5 do not divide them)
def test_refuses_worlds_that_do_not_tile_the_lanes(apw):
    with pytest.raises(ValueError, match="agents_per_world must be in 1..64 and divide the lane count 8"):
        bare_engine().episode_outcomes(_flags(), _flags(), _counts(), agents_per_world=apw)


def test_refuses_a_world_form_that_is_not_whole():
    info = torch.zeros(3, N, 2, dtype=torch.int32)
    latch = torch.zeros(N, dtype=torch.uint8)
    with pytest.raises(ValueError, match="runs once per step: k must be 1"):
        bare_engine().episode_outcomes(_flags(3), _flags(3), _counts(), info=info, agents_per_world=4, world_reset=_flags(), world_latch=latch)
    with pytest.raises(ValueError, match="world_reset .* and world_latch are required"):
        bare_engine().episode_outcomes(_flags(), _flags(), _counts(), agents_per_world=4, world_latch=latch)
    with pytest.raises(ValueError, match="world_reset .* and world_latch are required"):
        bare_engine().episode_outcomes(_flags(), _flags(), _counts(), agents_per_world=4, world_reset=_flags())
    with pytest.raises(ValueError, match="world_reset must be None with agents_per_world == 1"):
        bare_engine().episode_outcomes(_flags(), _flags(), _counts(), world_reset=_flags())


def test_checks_its_tensors():
    eng = bare_engine()
    with pytest.raises(ValueError, match=r"truncated must be a contiguous torch.bool/torch.uint8 tensor of shape \(3, 8\)"):
        eng.episode_outcomes(_flags(3), _flags(2), _counts(), info=torch.zeros(3, N, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"counts must be a contiguous int64 tensor of shape \(2, 16\)"):
        eng.episode_outcomes(_flags(), _flags(), _counts(1), n_groups=2)
    with pytest.raises(ValueError, match=r"counts must be a contiguous int64 tensor"):
        eng.episode_outcomes(_flags(), _flags(), _counts().double())
    with pytest.raises(ValueError, match=r"info must be a contiguous int32 tensor of shape \(3, 8, 2\)"):
        eng.episode_outcomes(_flags(3), _flags(3), _counts(), info=torch.zeros(3, N, 2))
    with pytest.raises(ValueError, match=r"group must be a contiguous int32 tensor of shape \(8,\)"):
        eng.episode_outcomes(_flags(), _flags(), _counts(), group=torch.zeros(N, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"valid must be a contiguous torch.bool/torch.uint8 tensor"):
        eng.episode_outcomes(_flags(), _flags(), _counts(), valid=torch.zeros(N))
    with pytest.raises(ValueError, match=r"outcome_out must be a contiguous uint8 tensor"):
        eng.episode_outcomes(_flags(), _flags(), _counts(), outcome_out=_flags())
    with pytest.raises(ValueError, match=r"world_latch must be a contiguous uint8 tensor"):
        eng.episode_outcomes(_flags(), _flags(), _counts(), agents_per_world=4, world_reset=_flags(), world_latch=_flags())


def test_the_fused_launch_has_no_outcomes_under_next_step():
    nn = torch.nn
    policy = MLPPolicy.from_torch(nn.Sequential(nn.Linear(21, 8), nn.Tanh(), nn.Linear(8, 4)), log_std=torch.zeros(4))
    eng = bare_engine("next_step")
    with pytest.raises(ValueError, match="fused=True with outcomes=True needs SAME_STEP"):
        eng.collect_rollout(policy, 4, fused=True, outcomes=True)
    with pytest.raises(ValueError, match="fused=True with outcomes=True needs SAME_STEP"):
        eng.rollout_policy(policy, 4, outcomes=True)
    assert eng._fused_policy(None, True) is False and eng._fused_policy(None, False) is True  # (QuadX-Hover: the fused launch is the default)
    assert bare_engine("same_step")._fused_policy(None, True) is True and bare_engine("same_step")._fused_policy(True, True) is True
    with pytest.raises(ValueError, match="outcomes must be a bool"):
        eng.collect_rollout(None, 4, outcomes=1)


def test_the_closed_loops_check_the_policy_behind_the_outcome_refusals():
    with pytest.raises(ValueError, match="policy must be a pyflyt_amd.MLPPolicy"):
        bare_engine("next_step").collect_rollout(None, 4, outcomes=True)
    with pytest.raises(ValueError, match="policy must be a pyflyt_amd.MLPPolicy"):
        bare_engine("off").rollout_policy_worlds(None, 4, 4, outcomes=True)


def test_an_opponent_pool_is_sized_and_grouped():
    lanes = torch.zeros(N, dtype=torch.bool)
    with pytest.raises(ValueError, match="a pool holds 1..16 policies, got 0"):
        bare_engine("off").rollout_policy_worlds(None, 4, 4, opponent=[], opponent_lanes=lanes)
    with pytest.raises(ValueError, match="a pool holds 1..16 policies, got 17"):
        bare_engine("off").rollout_policy_worlds(None, 4, 4, opponent=[None] * 17, opponent_lanes=lanes)
    with pytest.raises(ValueError, match="a pool of 2 needs group .* and n_groups = 2"):
        bare_engine("off").rollout_policy_worlds(None, 4, 4, opponent=[None, None], opponent_lanes=lanes)

"""pf_policy_pool_plan / pf_policy_act_pool without a GPU: the header's prototypes, the export list, the binding's argument types, the
size function, the library's refusals that need no device, and every ValueError the engine and the façades raise before a launch --
on an engine made without __init__ (tests/bare_engine.py) and on façades made without __init__ around one."""
import ctypes as C
import re

import pytest
import torch

from bare_engine import N, bare_engine
from pyflyt_amd import _lib as L
from pyflyt_amd import MLPPolicy
from pyflyt_amd.gym_envs import QuadXHoverVecEnv
from pyflyt_amd.pz_envs import MAFixedwingDogfightEnv


def policy(D=21, A=4, hidden=8):
    nn = torch.nn
    return MLPPolicy.from_torch(nn.Sequential(nn.Linear(D, hidden), nn.Tanh(), nn.Linear(hidden, A)), log_std=torch.zeros(A))


# ---------------------------------------------------------------------------------------------- the C surface
def test_header_declares_the_constant_and_the_prototypes():
    text = " ".join(open(L.HEADER_PATH).read().split())
    assert re.search(r"#define\s+PF_POLICY_POOL_MAX\s+17\b", text) and L.PF_POLICY_POOL_MAX == 17 == L.PF_OUTCOME_MAX_GROUPS + 1
    assert "size_t pf_policy_pool_plan_bytes(int n_rows, int n_policies);" in text
    assert "int pf_policy_pool_plan(pf_ctx* ctx, const int32_t* row_policy, int n_policies, void* plan, size_t plan_bytes, void* stream);" in text
    assert ("int pf_policy_act_pool(pf_ctx* ctx, const pf_policy* policies, int n_policies, const void* plan, size_t plan_bytes, "
            "float* actions_out, uint32_t step_index, void* stream);") in text
    assert re.search(r"#define\s+PF_ABI_VERSION\s+10\b", text)  # (new functions only)


def test_exported_and_bound():
    for name in ("pf_policy_pool_plan_bytes", "pf_policy_pool_plan", "pf_policy_act_pool"):
        assert name in L.EXPORTS
    lib = L.lib()  # (loads the library: every name of EXPORTS must be there)
    assert lib.pf_policy_pool_plan_bytes.argtypes == [C.c_int, C.c_int] and lib.pf_policy_pool_plan_bytes.restype == C.c_size_t
    assert lib.pf_policy_pool_plan.argtypes == [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    assert lib.pf_policy_act_pool.argtypes == [C.c_void_p, C.POINTER(L.PfPolicy), C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p]
    assert lib.pf_sizeof_policy() == C.sizeof(L.PfPolicy) == 88  # (pf_policy as it was: 17 blocks are 1 496 bytes of kernel arguments)


def test_plan_bytes():
    size = L.lib().pf_policy_pool_plan_bytes
    for n, p in ((0, 1), (-1, 1), (-2 ** 31, 4), (64, 0), (64, -1), (64, 18), (0, 0), (1000, 2 ** 31 - 1)):
        assert size(n, p) == 0, (n, p)
    for n in (1, 63, 64, 65, 1000, 65536, 2 ** 31 - 1):
        for p in range(1, 18):
            assert size(n, p) > 0
            assert size(n, p) >= 4 * (n + p)  # (room for every row's index and a word per policy at the least)
            if p < 17:
                assert size(n, p + 1) >= size(n, p)
    ns = [1, 2, 63, 64, 65, 127, 128, 129, 1000, 4096, 65535, 65536, 65537, 2 ** 31 - 1]
    for p in (1, 4, 17):
        sizes = [size(n, p) for n in ns]
        assert sizes == sorted(sizes)
    assert all(size(n + 1, 3) >= size(n, 3) for n in range(1, 400))


def test_the_library_refuses_null_arguments_before_any_device_work():
    lib = L.lib()
    q = (L.PfPolicy * 2)()
    assert lib.pf_policy_pool_plan(None, None, 1, None, 0, None) == L.ERR_ARG
    assert b"pf_policy_pool_plan" in lib.pf_last_error(None) and b"ctx" in lib.pf_last_error(None)
    assert lib.pf_policy_act_pool(None, q, 2, None, 0, None, 0, None) == L.ERR_ARG
    assert b"pf_policy_act_pool" in lib.pf_last_error(None) and b"ctx" in lib.pf_last_error(None)


# ---------------------------------------------------------------------------------------------- the engine
@pytest.mark.parametrize("p", [0, 18, -1, 2.0, True])
def test_plan_refuses_a_pool_size_outside_the_block(p):
    with pytest.raises(ValueError, match=r"n_policies must be an int in 1..17"):
        bare_engine().policy_pool_plan(torch.zeros(N, dtype=torch.int32), p)


def test_plan_checks_row_policy():
    eng = bare_engine()
    with pytest.raises(ValueError, match=r"row_policy must be a contiguous int32 tensor of shape \(8,\)"):
        eng.policy_pool_plan(torch.zeros(N, dtype=torch.int64), 2)
    with pytest.raises(ValueError, match=r"row_policy must be a contiguous int32 tensor of shape \(8,\)"):
        eng.policy_pool_plan(torch.zeros(N + 1, dtype=torch.int32), 2)
    with pytest.raises(ValueError, match=r"row_policy must be a contiguous int32 tensor of shape \(8,\)"):
        eng.policy_pool_plan(torch.zeros(2 * N, dtype=torch.int32)[::2], 2)
    with pytest.raises(ValueError, match="row_policy is required"):
        eng.policy_pool_plan(None, 2)


def test_act_pool_checks_the_pool_and_the_plan():
    eng = bare_engine()
    size = L.lib().pf_policy_pool_plan_bytes
    plan = torch.zeros(size(N, 2), dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"policies: a pool holds 1..17 policies, got 0"):
        eng.policy_act_pool([], plan)
    with pytest.raises(ValueError, match=r"policies: a pool holds 1..17 policies, got 18"):
        eng.policy_act_pool([policy()] * 18, plan)
    with pytest.raises(ValueError, match=r"policies: a pool holds 1..17 policies, got MLPPolicy"):
        eng.policy_act_pool(policy(), plan)
    with pytest.raises(ValueError, match="policy must be a pyflyt_amd.MLPPolicy"):
        eng.policy_act_pool([policy(), None], plan)
    with pytest.raises(ValueError, match=r"layers\[0\].weight reads 20 inputs, the env observes 21"):
        eng.policy_act_pool([policy(), policy(D=20)], plan)
    with pytest.raises(ValueError, match="the last layer writes 6 outputs, the env's action width is 4"):
        eng.policy_act_pool([policy(A=6), policy()], plan)
    # a plan of the wrong size: made for another pool size, for another n, no tensor, another dtype
    assert size(N, 3) != size(N, 2)
    with pytest.raises(ValueError, match=rf"plan must be a contiguous uint8 tensor of shape \({size(N, 3)},\)"):
        eng.policy_act_pool([policy()] * 3, plan)
    with pytest.raises(ValueError, match=r"plan must be a contiguous uint8 tensor"):
        eng.policy_act_pool([policy()] * 2, torch.zeros(size(N + 64, 2), dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"plan must be a contiguous uint8 tensor"):
        eng.policy_act_pool([policy()] * 2, plan.view(torch.int8))
    with pytest.raises(ValueError, match="plan is required"):
        eng.policy_act_pool([policy()] * 2, None)


# ---------------------------------------------------------------------------------------------- the stepwise loop with a list
@pytest.mark.parametrize("count", [0, 17])
def test_rollout_policy_steps_sizes_its_list(count):
    with pytest.raises(ValueError, match=rf"policy: a pool holds 1..16 policies, got {count}"):
        bare_engine().rollout_policy_steps([policy()] * count, 4, group=torch.zeros(N, dtype=torch.int32), n_groups=max(count, 1))


def test_rollout_policy_steps_checks_group_and_the_policies():
    eng, group = bare_engine(), torch.zeros(N, dtype=torch.int32)
    with pytest.raises(ValueError, match=r"a pool of 2 needs group .* and n_groups = 2"):
        eng.rollout_policy_steps([policy()] * 2, 4)
    with pytest.raises(ValueError, match=r"a pool of 2 needs group .* and n_groups = 2"):
        eng.rollout_policy_steps([policy()] * 2, 4, group=group, n_groups=3)
    with pytest.raises(ValueError, match=r"a pool of 2 needs group .* and n_groups = 2"):
        eng.rollout_policy_steps([policy()] * 2, 4, n_groups=2)
    with pytest.raises(ValueError, match=r"group must be a contiguous int32 tensor of shape \(8,\)"):
        eng.rollout_policy_steps([policy()] * 2, 4, group=group.long(), n_groups=2)
    with pytest.raises(ValueError, match=r"group must be a contiguous int32 tensor of shape \(8,\)"):
        eng.rollout_policy_steps([policy()] * 2, 4, group=torch.zeros(N - 1, dtype=torch.int32), n_groups=2)
    with pytest.raises(ValueError, match="policy must be a pyflyt_amd.MLPPolicy"):
        eng.rollout_policy_steps([policy(), "no policy"], 4, group=group, n_groups=2)
    with pytest.raises(ValueError, match=r"layers\[0\].weight reads 35 inputs, the env observes 21"):
        eng.rollout_policy_steps([policy(), policy(D=35)], 4, group=group, n_groups=2)
    with pytest.raises(ValueError, match="k_steps must be >= 1"):
        eng.rollout_policy_steps([policy()], 0)
    with pytest.raises(ValueError, match="needs an auto-reset mode"):
        bare_engine("off").rollout_policy_steps([policy()], 4)


# ---------------------------------------------------------------------------------------------- the world loop
def test_pooled_needs_an_opponent():
    lanes = torch.zeros(N, dtype=torch.bool)
    with pytest.raises(ValueError, match="pooled=True needs an opponent"):
        bare_engine("off").rollout_policy_worlds(policy(), 4, 4, pooled=True)
    with pytest.raises(ValueError, match="pooled=True needs an opponent"):
        bare_engine("off").collect_rollout_worlds(policy(), 4, 4, pooled=True)
    with pytest.raises(ValueError, match="pooled must be a bool"):
        bare_engine("off").rollout_policy_worlds(policy(), 4, 4, opponent=policy(), opponent_lanes=lanes, pooled=1)


@pytest.mark.parametrize("count", [0, 17])
def test_a_pooled_opponent_pool_is_sized(count):
    lanes = torch.zeros(N, dtype=torch.bool)
    with pytest.raises(ValueError, match=rf"a pool holds 1..16 policies, got {count}"):
        bare_engine("off").rollout_policy_worlds(policy(), 4, 4, opponent=[policy()] * count, opponent_lanes=lanes, pooled=True)


def test_a_pooled_world_loop_checks_its_tensors_and_policies():
    lanes, group = torch.zeros(N, dtype=torch.bool), torch.zeros(N, dtype=torch.int32)
    with pytest.raises(ValueError, match=r"a pool of 2 needs group .* and n_groups = 2"):
        bare_engine("off").rollout_policy_worlds(policy(), 4, 4, opponent=[policy()] * 2, opponent_lanes=lanes, pooled=True)
    with pytest.raises(ValueError, match=r"group must be a contiguous int32 tensor of shape \(8,\)"):
        bare_engine("off").rollout_policy_worlds(policy(), 4, 4, opponent=[policy()] * 2, opponent_lanes=lanes, group=group.long(), n_groups=2, pooled=True)
    with pytest.raises(ValueError, match="opponent and opponent_lanes come together"):
        bare_engine("off").rollout_policy_worlds(policy(), 4, 4, opponent=policy(), opponent_lanes=None, pooled=True)
    with pytest.raises(ValueError, match=r"opponent_lanes must be a contiguous torch.bool/torch.uint8 tensor of shape \(8,\)"):
        bare_engine("off").rollout_policy_worlds(policy(), 4, 4, opponent=policy(), opponent_lanes=lanes.float(), pooled=True)
    with pytest.raises(ValueError, match=r"layers\[0\].weight reads 22 inputs, the env observes 21"):
        bare_engine("off").rollout_policy_worlds(policy(), 4, 4, opponent=[policy(), policy(D=22)], opponent_lanes=lanes, group=group, n_groups=2, pooled=True)


# ---------------------------------------------------------------------------------------------- the façades
def hover_env(num_envs=N):
    """A QuadXHoverVecEnv that has been reset, without its __init__: what rollout() and collect() read before they reach the engine."""
    env = object.__new__(QuadXHoverVecEnv)
    env.engine, env.num_envs, env.device, env._needs_reset, env._policy_step = bare_engine(), num_envs, torch.device("cpu"), False, 0
    return env


@pytest.mark.parametrize("count", [0, 17])
def test_the_vector_env_sizes_its_list(count):
    with pytest.raises(ValueError, match=rf"policy: a pool holds 1..16 policies and at most one per env \(8\), got {count}"):
        hover_env().rollout([policy()] * count, 4)


def test_the_vector_env_wants_an_env_per_policy():
    with pytest.raises(ValueError, match=r"at most one per env \(8\), got 9"):
        hover_env().rollout([policy()] * 9, 4)


def test_the_vector_env_refuses_the_fused_launch_for_a_list_and_a_group_without_one():
    with pytest.raises(ValueError, match="fused=True with a list of policies"):
        hover_env().rollout([policy()] * 2, 4, fused=True)
    with pytest.raises(ValueError, match="fused must be None, True or False"):
        hover_env().rollout([policy()] * 2, 4, fused=1)
    with pytest.raises(ValueError, match="group comes with a list of policies"):
        hover_env().rollout(policy(), 4, group=torch.zeros(N, dtype=torch.int32))


def test_the_vector_env_checks_group_and_the_policies():
    with pytest.raises(ValueError, match=r"group must be a contiguous int32 tensor of shape \(8,\)"):
        hover_env().rollout([policy()] * 2, 4, group=torch.zeros(N, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"group must be a contiguous int32 tensor of shape \(8,\)"):
        hover_env().rollout([policy()] * 2, 4, group=torch.zeros(N, 1, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"layers\[0\].weight reads 20 inputs, the env observes 21"):
        hover_env().rollout([policy(), policy(D=20)], 4)
    with pytest.raises(ValueError, match="the last layer writes 7 outputs, the env's action width is 4"):
        hover_env().rollout([policy(A=7)], 4)


def test_the_default_group_is_near_equal_contiguous_segments():
    env = hover_env()
    assert env._pool_args([policy()] * 3, None, None)["group"].tolist() == [0, 0, 0, 1, 1, 1, 2, 2]  # (strong_shard: the remainder goes to the first ranks)
    assert env._pool_args([policy()] * 8, None, None)["group"].tolist() == list(range(8))
    args = env._pool_args([policy()], False, None)
    assert args["n_groups"] == 1 and args["group"].tolist() == [0] * 8 and args["group"].dtype == torch.int32


def test_collect_refuses_a_list():
    with pytest.raises(ValueError, match="collect\\(\\) takes one policy, not a list: a batch has one behaviour policy"):
        hover_env().collect([policy()] * 2, lambda o: o[:, 0], 4)


def test_the_dogfight_refuses_pooled_without_an_opponent():
    env = object.__new__(MAFixedwingDogfightEnv)
    env.engine, env.num_envs, env.num_possible_agents, env._needs_reset, env._policy_step = bare_engine("off"), 2, 4, False, 0
    with pytest.raises(ValueError, match="pooled=True needs an opponent"):
        env.rollout(policy(), 4, pooled=True)
    with pytest.raises(ValueError, match="pooled=True needs an opponent"):
        env.collect(policy(), lambda o: o[:, 0], 4, pooled=True)

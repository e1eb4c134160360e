"""pf_traj_stats_masked's host side: the header / binding, the refusals of BatchEngine.traj_stats(valid=...) and of the multi-agent
collect(stats=..., normalize_reward=...) that need no device."""
import ctypes as C
import os
import re

import pytest
import torch

from bare_engine import bare_engine
from pyflyt_amd import MLPPolicy
from pyflyt_amd import _lib as L
from pyflyt_amd.pz_envs.ma_fixedwing_dogfight import MAFixedwingDogfightEnv
from pyflyt_amd.pz_envs.ma_quadx_hover import MAQuadXHoverEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, K = 8, 5


def test_header_declares_the_masked_entry_points():
    text = open(os.path.join(ROOT, "include", "pyflyt_amd.h")).read()
    assert re.search(r"typedef\s+struct\s+pf_traj_stats_masked_args\s*\{", text)
    assert re.search(r"size_t\s+pf_sizeof_traj_stats_masked\s*\(\s*void\s*\)", text)
    assert re.search(r"int\s+pf_traj_stats_masked\s*\(\s*pf_ctx\s*\*\s*ctx\s*,\s*const\s+pf_traj_stats_masked_args\s*\*\s*a\s*,\s*int\s+k_steps\s*,"
                     r"\s*void\s*\*\s*stream\s*\)", text)
    assert "pf_traj_stats_masked" in L.EXPORTS and "pf_sizeof_traj_stats_masked" in L.EXPORTS
    assert L.PF_ABI_VERSION == 10


def test_sizeof_the_masked_block_and_of_the_existing_ones():
    # pf_traj_stats_args with `valid` where episode_start stood
    assert [f[0] for f in L.PfTrajStatsMasked._fields_] == [("valid" if f[0] == "episode_start" else f[0]) for f in L.PfTrajStats._fields_]
    assert C.sizeof(L.PfTrajStatsMasked) == 14 * C.sizeof(C.c_void_p)
    if not os.path.exists(L.LIB_PATH):
        pytest.fail(f"{L.LIB_PATH} is not built")
    lib = C.CDLL(L.LIB_PATH)
    for f in ("pf_sizeof_traj_stats_masked", "pf_sizeof_traj_stats", "pf_sizeof_gae", "pf_sizeof_world_sync"):
        getattr(lib, f).restype = C.c_size_t
    assert lib.pf_sizeof_traj_stats_masked() == C.sizeof(L.PfTrajStatsMasked)
    assert hasattr(lib, "pf_traj_stats_masked")
    # the existing blocks are as they were
    assert lib.pf_sizeof_traj_stats() == C.sizeof(L.PfTrajStats) == 14 * C.sizeof(C.c_void_p)
    assert lib.pf_sizeof_gae() == C.sizeof(L.PfGae) and lib.pf_sizeof_world_sync() == C.sizeof(L.PfWorldSync)


def good():
    return dict(reward=torch.zeros(K, N), terminated=torch.zeros(K, N, dtype=torch.bool), truncated=torch.zeros(K, N, dtype=torch.bool))


@pytest.mark.parametrize("mode", ["next_step", "same_step", "off"])
@pytest.mark.parametrize("change, fragment", [
    (dict(valid=torch.ones(K, N + 1, dtype=torch.bool)), "valid must be a contiguous torch.bool/torch.uint8 tensor of shape (5, 8)"),
    (dict(valid=torch.ones(K - 1, N, dtype=torch.uint8)), "valid must be a contiguous torch.bool/torch.uint8 tensor of shape (5, 8)"),
    (dict(valid=torch.ones(N, dtype=torch.bool)), "valid must be a contiguous torch.bool/torch.uint8 tensor of shape (5, 8)"),
    (dict(valid=torch.ones(K, N)), "valid must be a contiguous torch.bool/torch.uint8"),
    (dict(valid=torch.ones(K, N, dtype=torch.int32)), "valid must be a contiguous torch.bool/torch.uint8"),
    (dict(valid=torch.ones(N, K, dtype=torch.bool).t()), "valid must be a contiguous torch.bool/torch.uint8"),
    (dict(valid=[[1] * N] * K), "valid must be a contiguous torch.bool/torch.uint8"),
])
def test_traj_stats_refuses_a_bad_valid(mode, change, fragment):
    with pytest.raises(ValueError) as e:
        bare_engine(mode).traj_stats(**good(), **change)
    assert fragment in str(e.value), str(e.value)


def test_traj_stats_refuses_valid_together_with_episode_start():
    with pytest.raises(ValueError, match="valid and episode_start do not come together"):
        bare_engine("next_step").traj_stats(**good(), episode_start=torch.zeros(N, dtype=torch.bool), valid=torch.ones(K, N, dtype=torch.bool))


@pytest.mark.parametrize("cls", [MAFixedwingDogfightEnv, MAQuadXHoverEnv])
def test_multi_agent_collect_refuses_options_that_are_no_bools(cls):
    env = object.__new__(cls)  # (never __init__: that needs a GPU; the refusals come before anything is launched)
    env._needs_reset = False
    g = torch.Generator().manual_seed(0)
    pol = MLPPolicy([(torch.randn(8, 21, generator=g), torch.zeros(8)), (torch.randn(4, 8, generator=g), torch.zeros(4))])
    with pytest.raises(ValueError, match="stats must be a bool"):
        env.collect(pol, lambda o: o[:, 0], 4, stats="yes")
    with pytest.raises(ValueError, match="normalize_reward must be a bool"):
        env.collect(pol, lambda o: o[:, 0], 4, normalize_reward=1)
    env._needs_reset = True
    with pytest.raises(RuntimeError, match="reset"):
        env.collect(pol, lambda o: o[:, 0], 4, stats=True)

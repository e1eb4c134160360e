"""pf_traj_stats's host side: the header / binding, the argument validation of BatchEngine.traj_stats and env.collect(stats=...) that
needs no device, RunningMoments on a hand-filled block, MLPPolicy.set_obs_stats."""
import ctypes as C
import os
import re

import pytest
import torch

from bare_engine import bare_engine
from pyflyt_amd import MLPPolicy, RunningMoments
from pyflyt_amd import _lib as L
from pyflyt_amd.gym_envs.vector_envs import QuadXHoverVecEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, K, D = 8, 5, 21


def test_header_declares_the_traj_stats_entry_points():
    text = open(os.path.join(ROOT, "include", "pyflyt_amd.h")).read()
    assert re.search(r"typedef\s+struct\s+pf_traj_stats_args\s*\{", text)
    assert re.search(r"size_t\s+pf_sizeof_traj_stats\s*\(\s*void\s*\)", text)
    assert re.search(r"int\s+pf_traj_stats\s*\(\s*pf_ctx\s*\*\s*ctx\s*,\s*const\s+pf_traj_stats_args\s*\*\s*a\s*,\s*int\s+k_steps\s*,\s*void\s*\*\s*stream\s*\)", text)
    assert "pf_traj_stats" in L.EXPORTS and "pf_sizeof_traj_stats" in L.EXPORTS
    assert L.PF_ABI_VERSION == 10


def test_sizeof_traj_stats_matches_the_parsed_mirror():
    assert [f[0] for f in L.PfTrajStats._fields_] == ["gamma", "reward", "terminated", "truncated", "episode_start", "obs", "carry_return",
                                                      "carry_length", "carry_disc", "ep_return_out", "ep_length_out", "summary", "ret_moments",
                                                      "obs_moments"]
    assert C.sizeof(L.PfTrajStats) == 14 * C.sizeof(C.c_void_p)  # (the float, padded to a pointer, and thirteen pointers)
    if not os.path.exists(L.LIB_PATH):
        pytest.fail(f"{L.LIB_PATH} is not built")
    lib = C.CDLL(L.LIB_PATH)
    lib.pf_sizeof_traj_stats.restype = C.c_size_t
    assert lib.pf_sizeof_traj_stats() == C.sizeof(L.PfTrajStats)
    assert hasattr(lib, "pf_traj_stats")


def good():
    return dict(reward=torch.zeros(K, N), terminated=torch.zeros(K, N, dtype=torch.bool), truncated=torch.zeros(K, N, dtype=torch.bool))


@pytest.mark.parametrize("change, fragment", [
    (dict(reward=torch.zeros(K, N + 1)), "reward must be a contiguous float32 tensor of shape (5, 8)"),
    (dict(reward=torch.zeros(K, N, dtype=torch.float64)), "reward must be a contiguous float32"),
    (dict(reward=torch.zeros(N)), "reward must be a float32 tensor of shape (k, 8)"),
    (dict(reward=[0.0] * N), "reward must be a float32 tensor of shape (k, 8)"),
    (dict(terminated=torch.zeros(K, N)), "terminated must be a contiguous torch.bool/torch.uint8"),
    (dict(terminated=None), "terminated is required"),
    (dict(truncated=torch.zeros(K - 1, N, dtype=torch.bool)), "truncated must be a contiguous torch.bool/torch.uint8 tensor of shape (5, 8)"),
    (dict(gamma=1.5), "gamma must be finite and in [0, 1]"),
    (dict(gamma=float("nan")), "gamma must be finite and in [0, 1]"),
    (dict(episode_start=torch.zeros(N)), "episode_start must be a contiguous torch.bool/torch.uint8 tensor of shape (8,)"),
    (dict(episode_start=torch.zeros(N + 1, dtype=torch.bool)), "episode_start must be"),
    (dict(obs=torch.zeros(K, N, D + 1)), "obs must be a contiguous float32 tensor of shape (5, 8, 21)"),
    (dict(obs=torch.zeros(K + 1, N, D)[:-1].transpose(0, 1)), "obs must be a contiguous float32"),
    (dict(obs=torch.zeros(K, N, D, dtype=torch.float64)), "obs must be a contiguous float32"),
    (dict(obs="rows"), "obs must be a float32 tensor of shape (k, 8, D)"),
])
def test_traj_stats_refusals_name_the_argument(change, fragment):
    kw = good()
    kw.update(change)
    with pytest.raises(ValueError) as e:
        bare_engine().traj_stats(**kw)
    assert fragment in str(e.value), str(e.value)


def test_traj_stats_refuses_episode_start_outside_next_step():
    for mode in ("same_step", "off"):
        with pytest.raises(ValueError, match="episode_start must be None outside NEXT_STEP"):
            bare_engine(mode).traj_stats(**good(), episode_start=torch.zeros(N, dtype=torch.bool))


def test_collect_refuses_options_that_are_no_bools():
    env = object.__new__(QuadXHoverVecEnv)
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


def test_running_moments_on_a_hand_filled_block():
    block = torch.tensor([4.0, 1.0, -2.0, 8.0, 1.0], dtype=torch.float64)  # count 4, mean (1, -2), M2 (8, 1)
    m = RunningMoments(block)
    assert m.dim == 2 and m.count.dtype == torch.float32 and float(m.count) == 4.0
    assert m.mean.dtype == torch.float32 and m.mean.tolist() == [1.0, -2.0]
    assert m.var.dtype == torch.float32 and m.var.tolist() == [2.0, 0.25]
    assert torch.allclose(m.std(), torch.tensor([2.0 + 1e-8, 0.25 + 1e-8]).sqrt()) and torch.allclose(m.std(eps=1.0), torch.tensor([3.0, 1.25]).sqrt())
    block[0] = 1.0  # fewer than two samples: variance 1
    assert m.var.tolist() == [1.0, 1.0]
    block.zero_()   # the empty state: mean 0, variance 1 -- a normaliser that does nothing
    assert float(m.count) == 0.0 and m.mean.tolist() == [0.0, 0.0] and m.var.tolist() == [1.0, 1.0]
    assert RunningMoments(torch.zeros(3, dtype=torch.float64)).dim == 1
    for bad in (torch.zeros(5), torch.zeros(4, dtype=torch.float64), torch.zeros(1, dtype=torch.float64), [0.0, 0.0, 0.0]):
        with pytest.raises(ValueError, match=r"block must be a float64 tensor of shape \(1 \+ 2 D,\)"):
            RunningMoments(bad)


def test_set_obs_stats_folds_like_the_constructor():
    g = torch.Generator().manual_seed(1)
    layers = [(torch.randn(8, D, generator=g), torch.randn(8, generator=g)), (torch.randn(4, 8, generator=g), torch.randn(4, generator=g))]
    mean, std = torch.randn(D, generator=g), torch.rand(D, generator=g) + 0.5
    built = MLPPolicy(layers, obs_mean=mean, obs_std=std)
    pol = MLPPolicy(layers)
    assert pol.obs_mean is None and pol.device_layers()[0][0] is layers[0][0]
    assert pol.set_obs_stats(mean, std) is pol
    for a, b in zip(pol.device_layers()[0], built.device_layers()[0]):
        assert torch.equal(a, b)
    assert pol.obs_mean is not mean and torch.equal(pol.obs_mean, mean) and torch.equal(pol.obs_std, std)
    keep = pol.obs_mean
    pol.set_obs_stats(mean + 1.0, std * 2.0)  # copied into the same tensors, folded again
    assert pol.obs_mean is keep and torch.equal(keep, mean + 1.0)
    again = MLPPolicy(layers, obs_mean=mean + 1.0, obs_std=std * 2.0)
    for a, b in zip(pol.device_layers()[0], again.device_layers()[0]):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="mean has 20 entries for an observation width of 21"):
        pol.set_obs_stats(torch.zeros(D - 1), std)
    with pytest.raises(ValueError, match="std must be float32"):
        pol.set_obs_stats(mean, std.double())

"""The launch sequence of the stepwise closed loops, as their docstrings promise it: per step pf_policy_act and pf_env_step on the
single-agent envs; on the multi-agent envs pf_policy_act, with an opponent its pf_policy_act (and the merge, a torch kernel, which is no
foreign call), then pf_env_step, pf_world_sync, pf_env_reset -- "four launches ... six with an opponent". For the length of one call the
engine's library is a proxy that writes down every foreign call with its arguments as plain integers and calls through; k = 3 steps
from step index 0xFFFFFFFE, so that the index wraps inside the call. One wavefront each: the bits are pinned elsewhere
(test_gpu_ma_collect, test_gpu_policy_act, test_gpu_gae)."""
import ctypes as C

import pytest
import torch

from pyflyt_amd import build_params
from pyflyt_amd.engine import BatchEngine
from pyflyt_amd.pz_envs import MAFixedwingDogfightEnv, MAQuadXHoverEnv
from test_gpu_ma_collect import make_policy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K, STEP0 = 3, 0xFFFFFFFE
SINGLE = ["pf_policy_act", "pf_env_step"]
WORLD = ["pf_policy_act", "pf_env_step", "pf_world_sync", "pf_env_reset"]
WORLD_OPPONENT = ["pf_policy_act", "pf_policy_act", "pf_env_step", "pf_world_sync", "pf_env_reset"]


def plain(a):
    """A foreign call's argument as an integer: an address for a pointer or a byref(), 0 for a null pointer."""
    if a is None or isinstance(a, int):
        return a or 0
    if isinstance(a, C.c_void_p):
        return a.value or 0
    return C.addressof(a._obj)


class Recorder:
    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)

        def call(*args):
            self.calls.append((name, tuple(plain(a) for a in args)))
            return fn(*args)

        return call


def recorded(eng, call):
    """(call()'s result, the foreign calls `eng` made meanwhile)."""
    rec = eng.lib = Recorder(eng.lib)
    try:
        return call(), rec.calls
    finally:
        eng.lib = rec.lib


def check(eng, calls, per_step, actions, tail=()):
    n, W = eng.n, eng.action_dim
    assert [c[0] for c in calls] == per_step * K + list(tail), [c[0] for c in calls]
    assert tuple(actions.shape) == (K, n, W) and actions.is_contiguous()
    acts = [args for name, args in calls if name == "pf_policy_act"]
    per = per_step.count("pf_policy_act")
    assert len(acts) == per * K
    for s in range(K):
        ctx, q, a, index, stream = acts[per * s]
        assert a == actions.data_ptr() + 4 * n * W * s, s
        assert index == (STEP0 + s) & 0xFFFFFFFF, s
        if per == 2:  # (the opponent's: the same step index, into the buffer the merge reads)
            ctx, q, a, index, stream = acts[per * s + 1]
            assert a == eng._opp_act.data_ptr() and index == (STEP0 + s) & 0xFFFFFFFF, s
    assert [(STEP0 + s) & 0xFFFFFFFF for s in range(K)] == [0xFFFFFFFE, 0xFFFFFFFF, 0]  # (the wrap is crossed)


@pytest.mark.parametrize("autoreset", ["next_step", "same_step"])
def test_single_agent_steps(autoreset):
    eng = BatchEngine(build_params("fixedwing", "waypoints", seed=11, autoreset=autoreset), 64, device=DEV)
    eng.env_reset()
    pol = make_policy(eng.obs_dim, eng.action_dim, 5)
    out, calls = recorded(eng, lambda: eng.rollout_policy_steps(pol, K, step_index0=STEP0))
    check(eng, calls, SINGLE, out[4])
    t, calls = recorded(eng, lambda: eng.collect_rollout(pol, K, step_index0=STEP0, fused=False))
    check(eng, calls, SINGLE, t["actions"])
    torch.cuda.synchronize()


@pytest.mark.parametrize("opponent", [False, True])
def test_dogfight_worlds(opponent):
    env = MAFixedwingDogfightEnv(team_size=2, num_envs=16, seed=11)
    env.reset(seed=11)
    eng = env.engine
    assert eng.n == 64
    pol = make_policy(eng.obs_dim, eng.action_dim, 5)
    opp = make_policy(eng.obs_dim, eng.action_dim, 6) if opponent else None
    per_step = WORLD_OPPONENT if opponent else WORLD
    env._policy_step = STEP0
    out, calls = recorded(eng, lambda: env.rollout(pol, K, opponent=opp))
    check(eng, calls, per_step, out[4])
    assert env._policy_step == (STEP0 + K) & 0xFFFFFFFF
    env._policy_step = STEP0
    batch, calls = recorded(eng, lambda: env.collect(pol, lambda o: o[:, 0], K, opponent=opp))
    check(eng, calls, per_step, batch["actions"], tail=["pf_gae"])
    assert env._policy_step == (STEP0 + K) & 0xFFFFFFFF
    torch.cuda.synchronize()


def test_hover_worlds():
    env = MAQuadXHoverEnv(num_envs=16, seed=11)
    env.reset(seed=11)
    eng = env.engine
    assert eng.n == 64 and env.num_possible_agents == 4
    pol = make_policy(eng.obs_dim, eng.action_dim, 5)
    env._policy_step = STEP0
    out, calls = recorded(eng, lambda: env.rollout(pol, K))
    check(eng, calls, WORLD, out[4])
    assert env._policy_step == (STEP0 + K) & 0xFFFFFFFF
    torch.cuda.synchronize()

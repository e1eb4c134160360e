"""The fixed call shape of the specialised QuadX one-step kernel (pyflyt_amd/csrc/quadx_fast.hpp: FIXED -- pf_env_step without a mask,
NEXT_STEP auto-reset, the task's default Aviary steps per env step (Hover 3, Waypoints 4), quaternion observations, dense reward,
all pinned at compile time) is the
general body with its control flow folded: a default context (pf_ctx_step_is_fixed() == 1) steps bit-identically to one built with
PF_NO_FIXED_STEP=1 (read at context creation), through spare resets, refills and resets without a spare. The same arithmetic: no
tolerance. pf_env_reset keeps the general kernel on both sides; the two share the state layout and interleave freely."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _pair(monkeypatch, task, noise, n, seed=5, **kw):
    """(default context, the same context with PF_NO_FIXED_STEP=1)"""
    from pyflyt_amd import build_params
    from pyflyt_amd.engine import BatchEngine

    def make(fixed):
        if fixed:
            monkeypatch.delenv("PF_NO_FIXED_STEP", raising=False)
        else:
            monkeypatch.setenv("PF_NO_FIXED_STEP", "1")
        eng = BatchEngine(build_params("quadx", task, noise=noise, seed=seed, **kw), n, device=DEV)
        assert eng.lib.pf_ctx_is_specialised(eng._ctx) == 1
        return eng

    a, b = make(True), make(False)
    monkeypatch.delenv("PF_NO_FIXED_STEP", raising=False)
    return a, b


def _same(a, b, ra, rb, where):
    for name, x, y in zip(("obs", "reward", "terminated", "truncated"), ra, rb):
        assert torch.equal(x, y), (name, where)
    assert torch.equal(a.state, b.state), ("state", where)


@pytest.mark.parametrize("n", [64, 192])  # one wave; three workgroups = three counter words of the refill cadence
@pytest.mark.parametrize("noise", ["philox", "off"])
@pytest.mark.parametrize("task", ["hover", "waypoints"])
def test_fixed_step_is_bit_identical_to_the_general_kernel(monkeypatch, task, noise, n):
    a, b = _pair(monkeypatch, task, noise, n)
    assert a.lib.pf_ctx_step_is_fixed(a._ctx) == 1 and a.step_is_fixed
    assert b.lib.pf_ctx_step_is_fixed(b._ctx) == 0 and not b.step_is_fixed
    assert torch.equal(a.env_reset(), b.env_reset()) and torch.equal(a.state, b.state)
    act = torch.empty(n, 4, device=DEV)
    restarts = torch.zeros(n, dtype=torch.int32, device=DEV)  # times a lane's step_count came back to 0
    refills = 0                                              # launches that left some lane a fresh spare
    for k in range(80):  # five refill periods (kSpareEvery = 16)
        a.sample_actions(act, k)
        had = a.state[7, :, 3].view(torch.int32) < 0  # bit 31 of the key word: the lane holds a prepared spare
        cnt = a.ints()[:, 0].clone()
        _same(a, b, a.env_step(act), b.env_step(act), (task, noise, n, k))
        restarts += ((a.ints()[:, 0] == 0) & (cnt > 0)).int()
        refills += int(bool(((a.state[7, :, 3].view(torch.int32) < 0) & ~had).any()))
    assert int(restarts.min()) >= 1, restarts  # every lane went through the reset path
    assert refills >= 1


@pytest.mark.parametrize("kw", [dict(agent_hz=60), dict(autoreset="same_step"), dict(angle_representation="euler"), dict(sparse_reward=True)],
                         ids=["ratio2", "same_step", "euler", "sparse"])
def test_outside_the_envelope_nothing_is_fixed(monkeypatch, kw):
    a, b = _pair(monkeypatch, "hover", "philox", 192, **kw)
    assert a.lib.pf_ctx_step_is_fixed(a._ctx) == 0 and b.lib.pf_ctx_step_is_fixed(b._ctx) == 0
    assert torch.equal(a.env_reset(), b.env_reset())
    act = torch.empty(192, 4, device=DEV)
    for k in range(24):
        a.sample_actions(act, k)
        _same(a, b, a.env_step(act), b.env_step(act), (kw, k))


@pytest.mark.parametrize("task", ["hover", "waypoints"])
def test_a_masked_reset_between_fixed_steps(monkeypatch, task):
    n = 192
    a, b = _pair(monkeypatch, task, "philox", n)
    assert a.step_is_fixed and not b.step_is_fixed
    assert torch.equal(a.env_reset(), b.env_reset())
    act = torch.empty(n, 4, device=DEV)
    mask = torch.arange(n, device=DEV) % 3 == 1
    for k in range(40):
        if k in (7, 20, 31):  # (a masked pf_env_reset runs the general kernel on both sides, on the state the fixed steps left)
            assert torch.equal(a.env_reset(mask), b.env_reset(mask)) and torch.equal(a.state, b.state), k
            assert bool((a.ints()[mask, 0] == 0).all())
        a.sample_actions(act, k)
        _same(a, b, a.env_step(act), b.env_step(act), (task, k))


def test_a_captured_fixed_step_replays_like_eager_steps(monkeypatch):
    """The refill cadence is device state: one captured fixed step replayed 40 times is 40 eager steps of the general kernel."""
    n = 192
    a, b = _pair(monkeypatch, "hover", "philox", n)
    assert a.step_is_fixed and not b.step_is_fixed
    assert torch.equal(a.env_reset(), b.env_reset())
    act = torch.empty(n, 4, device=DEV)
    for k in range(3):  # (warm up outside the capture)
        a.sample_actions(act, k)
        _same(a, b, a.env_step(act), b.env_step(act), k)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            a.env_step(act)
        stream.synchronize()
    ends = 0
    for k in range(40):
        graph.replay()
        rb = b.env_step(act)
        torch.cuda.synchronize()
        _same(a, b, (a.obs, a.reward, a.terminated, a.truncated), rb, k)
        ends += int((rb[2] | rb[3]).sum())
    assert ends > 0

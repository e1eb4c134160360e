"""The paths of the fixed one-step QuadX kernel (pyflyt_amd/csrc/quadx_fast.hpp: FIXED) that random actions from a fresh reset meet
rarely or never within a short test, each forced by writing the lanes' state: lanes that leave the dome in the 1st, 2nd, .. Aviary
step of an env step (the straight-line calm path's exits, and the run-time loop's in a wave with a low lane), restarts with and
without a prepared spare in one wave across a refill, attitudes on every branch of the reward's and the observation's roll / pitch
(the packed atan2 pair), and a captured Waypoints step replayed across a refill. Every check is torch.equal of a default context
(step_is_fixed) against one created under PF_NO_FIXED_STEP=1, on obs, reward, terminated, truncated and the whole state: the same
arithmetic, no tolerance."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [64, 192, 100]  # one wave; three workgroups; a full and a partial wave
DT = 1.0 / 240.0        # the physics tick; two ticks per Aviary step, 3 (Hover) / 4 (Waypoints) Aviary steps per env step
RATIO = {"hover": 3, "waypoints": 4}
DOME = {"hover": 3.0, "waypoints": 5.0}
F_TERMINATED, F_TRUNCATED = 1, 2


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
    assert a.step_is_fixed and not b.step_is_fixed
    return a, b


def _same(a, b, ra, rb, where):
    for name, x, y in zip(("obs", "reward", "terminated", "truncated"), ra, rb):
        assert torch.equal(x, y), (name, where)
    assert torch.equal(a.state, b.state), ("state", where)


def _reset(a, b):
    assert torch.equal(a.env_reset(), b.env_reset()) and torch.equal(a.state, b.state)


def _lanes(n, offset):
    """Lanes spread over every wave of the batch (the partial one included), shifted by `offset`."""
    return torch.tensor([x + offset for x in (5, 17, 40, 70, 90, 130, 180) if x + offset < n], device=DEV)


def _put_outside(eng, task, lanes):
    """These lanes beyond the dome, at rest: they terminate in the first Aviary step of the next env step."""
    eng.state[0, lanes, 0] = DOME[task] + 0.5
    eng.state[2, lanes, 0:3] = 0.0


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("noise", ["philox", "off"])
@pytest.mark.parametrize("task", ["hover", "waypoints"])
def test_lanes_that_stop_in_the_middle_of_an_env_step(monkeypatch, task, noise, n):
    """Group k = 1 .. ratio flies outward along x at 12 m/s (0.05 m a tick, 0.1 m an Aviary step) from half an Aviary step's travel
    inside the point where |p| crosses the dome after k Aviary steps: it is inside after k - 1 of them, outside after k, terminates
    there and stops integrating, so x has advanced by 2k ticks of v dt. The margin is half an Aviary step, 0.05 m, against what the
    estimate leaves out: gravity over eight ticks moves z by 5 mm (the crossing point by 1 mm), drag takes a few percent of v."""
    a, b = _pair(monkeypatch, task, noise, n)
    _reset(a, b)
    speed, ratio = 12.0, RATIO[task]
    groups, x0s = [], []
    for k in range(1, ratio + 1):
        lanes = _lanes(n, k)
        z = a.state[0, lanes, 2]
        x0 = torch.sqrt(DOME[task] ** 2 - z * z) - (k - 0.5) * (2.0 * speed * DT)
        for eng in (a, b):
            eng.state[0, lanes, 0] = x0
            eng.state[0, lanes, 1] = 0.0
            eng.state[2, lanes, 0] = speed
            eng.state[2, lanes, 1:3] = 0.0
        groups.append(lanes)
        x0s.append(x0)
    if n == 192:  # a lane near the floor: its wave is not calm and takes the run-time loop, with the same exits in it
        for eng in (a, b):
            eng.state[0, 150, 2] = 0.2
    assert torch.equal(a.state, b.state)
    act = torch.zeros(n, 4, device=DEV)
    _same(a, b, a.env_step(act), b.env_step(act), (task, noise, n))
    for k, lanes, x0 in zip(range(1, ratio + 1), groups, x0s):
        assert bool(a.terminated[lanes].all()), (k, a.terminated[lanes])
        ticks = (a.state[0, lanes, 0] - x0) / (speed * DT)
        print(f"{task} {noise} n={n} group {k}: x advanced by {ticks.tolist()} ticks of v dt (expected {2 * k})")
        assert bool(((ticks - 2 * k).abs() < 0.5).all()), (k, ticks)
    flying = torch.ones(n, dtype=torch.bool, device=DEV)
    flying[torch.cat(groups)] = False
    if n == 192:
        flying[150] = False
    assert not bool(a.terminated[flying].any())  # (the others fly on)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("noise", ["philox", "off"])
@pytest.mark.parametrize("task", ["hover", "waypoints"])
def test_every_restart_kind_in_one_wave(monkeypatch, task, noise, n):
    """After pf_env_reset every lane holds a spare. Lanes A leave the dome in step 0 and restart from their spares in step 1; half of
    them leave again in step 2, together with lanes B for the first time, so step 3 restarts lanes without a spare (generated
    cooperatively) and lanes with one (copied) in the same waves, next to lanes that fly on. Twenty steps: the refill of step 15
    (kSpareEvery = 16) is in them."""
    a, b = _pair(monkeypatch, task, noise, n)
    _reset(a, b)
    A, B = _lanes(n, 0), _lanes(n, 7)
    act = torch.empty(n, 4, device=DEV)
    with_spare = without_spare = refills = 0
    for k in range(20):
        if k == 0:
            for eng in (a, b):
                _put_outside(eng, task, A)
        if k == 2:
            for eng in (a, b):
                _put_outside(eng, task, torch.cat([A[::2], B]))
        a.sample_actions(act, k)
        ints = a.ints()
        restarting = (ints[:, 1] & (F_TERMINATED | F_TRUNCATED)) != 0  # NEXT_STEP: these lanes restart in the step at hand
        had = a.state[7, :, 3].view(torch.int32) < 0                   # bit 31 of the key word: the lane holds a prepared spare
        with_spare += int((restarting & had).sum())
        without_spare += int((restarting & ~had).sum())
        _same(a, b, a.env_step(act), b.env_step(act), (task, noise, n, k))
        assert bool((a.ints()[restarting, 0] == 0).all())  # (a restarting lane does not step: its count is back at 0)
        refills += int(bool(((a.state[7, :, 3].view(torch.int32) < 0) & ~had).any()))
        if k == 3:
            assert with_spare >= len(A) + len(B) and without_spare >= len(A[::2]), (with_spare, without_spare)
    assert with_spare > 0 and without_spare > 0 and refills >= 1, (with_spare, without_spare, refills)


def _quat(roll, pitch, yaw):
    """getQuaternionFromEuler in float64, (x, y, z, w)."""
    cr, sr, cp, sp, cy, sy = (f(0.5 * t) for t in (roll, pitch, yaw) for f in (math.cos, math.sin))
    return [sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("noise", ["philox", "off"])
def test_attitudes_on_every_branch_of_roll_and_pitch(monkeypatch, noise, n):
    """Hover's reward takes atan2(R21, R22) and asin(-R20), the observation their half angles, both behind the gimbal test
    |R20| >= 0.99999 (pitch within 4.47e-3 rad of +-90 deg): roll and pitch in all four sign combinations, |roll| below and above
    90 deg, pitch on both sides of the gimbal threshold and within 1e-3 rad of +-90 deg, and the identity."""
    a, b = _pair(monkeypatch, "hover", noise, n)
    _reset(a, b)
    quats = [[0.0, 0.0, 0.0, 1.0]]
    for roll in (0.4, 2.0, 3.0):  # (2.0, 3.0: |roll| > 90 deg, R22 < 0)
        for pitch in (0.3, 1.2):
            for sr in (1.0, -1.0):
                for sp in (1.0, -1.0):
                    quats.append(_quat(sr * roll, sp * pitch, 0.7))
    for d in (2e-4, 1e-3, 4.3e-3, 4.6e-3, 6e-3):  # distance of the pitch from 90 deg; the threshold is at 4.47e-3
        for sp in (1.0, -1.0):
            for roll in (0.5, -2.5):
                quats.append(_quat(roll, sp * (0.5 * math.pi - d), -1.1))
    q = torch.tensor(quats, dtype=torch.float32, device=DEV)
    q64 = q.double()
    sarg = 2.0 * (q64[:, 3] * q64[:, 1] - q64[:, 0] * q64[:, 2]) / (q64 * q64).sum(1)
    assert int((sarg.abs() >= 0.99999).sum()) >= 8 and int(((sarg.abs() < 0.99999) & (sarg.abs() > 0.9999)).sum()) >= 4  # both sides
    lanes = (torch.arange(len(quats), device=DEV) * 7 + 3) % n  # (7 is coprime to 64, 100 and 192: distinct lanes in every wave)
    assert len(set(lanes.tolist())) == len(quats)
    for eng in (a, b):
        eng.state[1, lanes, :] = q
    act = torch.zeros(n, 4, device=DEV)
    _same(a, b, a.env_step(act), b.env_step(act), (noise, n))
    assert bool(torch.isfinite(a.reward).all()) and bool(torch.isfinite(a.obs).all())


def test_a_captured_waypoints_step_replays_like_eager_steps(monkeypatch):
    """The refill cadence is device state: one captured fixed Waypoints step replayed 40 times (two refills) is 40 eager steps of the
    general kernel."""
    n = 192
    a, b = _pair(monkeypatch, "waypoints", "philox", n)
    _reset(a, b)
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
    ends = refills = 0
    for k in range(40):
        had = b.state[7, :, 3].view(torch.int32) < 0
        graph.replay()
        rb = b.env_step(act)
        torch.cuda.synchronize()
        _same(a, b, (a.obs, a.reward, a.terminated, a.truncated), rb, k)
        ends += int((rb[2] | rb[3]).sum())
        refills += int(bool(((b.state[7, :, 3].view(torch.int32) < 0) & ~had).any()))
    assert ends > 0 and refills >= 1, (ends, refills)

"""Shared-world Aviary (drones_per_world = K > 1) without a GPU: the limits are refused before any engine is built, the parameter
block carries K, and the fp64 oracle shows the drag-gate gap the GPU test relies on."""
import numpy as np
import pytest

from pyflyt_amd import build_params
from pyflyt_amd.core import Aviary
from pyflyt_amd.core.aviary import AviaryInitException


def _pos(n):
    return np.stack([np.arange(n) * 2.0, np.zeros(n), np.ones(n)], axis=1), np.zeros((n, 3))


@pytest.fixture
def no_engine(monkeypatch):
    """Any attempt to build an engine fails the test: the checks must fire first (and so run on a machine without a GPU)."""
    import pyflyt_amd.core.aviary as A

    def boom(*a, **k):
        raise AssertionError("an engine was built before the shared-world checks")

    monkeypatch.setattr(A, "BatchEngine", boom)


@pytest.mark.parametrize("n,K,match", [(6, 4, "must divide"), (6, 3, "1, 2, 4 or 8"), (32, 16, "1, 2, 4 or 8"), (4, 0, "1, 2, 4 or 8")])
def test_world_size_limits(no_engine, n, K, match):
    pos, orn = _pos(n)
    with pytest.raises(AviaryInitException, match=match):
        Aviary(pos, orn, drone_type="quadx", drones_per_world=K)


def test_rocket_refused(no_engine):
    pos, orn = _pos(4)
    with pytest.raises(AviaryInitException, match="not the rocket"):
        Aviary(pos, orn, drone_type="rocket", drones_per_world=2)


def test_primitive_drone_refused(no_engine):
    pos, orn = _pos(4)
    with pytest.raises(AviaryInitException, match="plain, unyawed box colliders"):
        Aviary(pos, orn, drone_type="quadx", drone_options=dict(drone_model="primitive_drone"), drones_per_world=2)


def test_wind_field_refused(no_engine):
    pos, orn = _pos(4)

    def field(np_random=None, **kw):  # (never called: the constructor refuses first)
        return lambda t, p: p * 0.0

    with pytest.raises(AviaryInitException, match="wind field"):
        Aviary(pos, orn, drone_type="quadx", wind_type=field, drones_per_world=2)


def test_mixed_aviary_refused(no_engine):
    pos, orn = _pos(4)
    with pytest.raises(AviaryInitException, match="MixedAviary"):
        Aviary(pos, orn, drone_type=["quadx", "fixedwing", "quadx", "fixedwing"], drones_per_world=2)


def test_build_params_carries_agents_per_world():
    assert build_params("quadx", "none", agents_per_world=4).agents_per_world == 4
    assert build_params("fixedwing", "none", agents_per_world=2).agents_per_world == 2
    assert build_params("quadx", "none").agents_per_world == 0  # (0 / 1: every drone alone, the library's default)


def test_oracle_drag_gate_gap():
    """The landing scene of tests/test_gpu_aviary_world.py on the oracle, stepped two ways: the whole world in one
    orc_world_aviary_step, and every drone as a world of its own (drones_per_world=1). Once the landing drone touches down, the world
    switches the flying drones' rotational drag off (quadx.py:509) and their spin stops decaying; alone, it keeps decaying. The gap
    must dwarf the one-step parity bound (1e-4 max(1, |w|)) for the GPU test to tell the two apart."""
    from aviary_world_scenes import SPIN, OracleAviaryWorlds, scene

    K, W = 4, 2
    pos, orn, vel, ang, sp = scene("landing", K, W)
    world = OracleAviaryWorlds("quadx", K, W, pos, orn, vel, ang, sp, -1)
    solo = OracleAviaryWorlds("quadx", K, W, pos, orn, vel, ang, sp, -1)
    fly = np.array([i for i in range(K * W) if i % K])
    touch, gap = None, 0.0
    for k in range(200):
        world.step()
        solo.step(solo=True)
        if touch is None and world.contact_step()[0]:
            touch = k
        if touch is not None:
            gap = max(gap, float(np.abs(world.states()[fly, 0] - solo.states()[fly, 0]).max()))
    bound = 1e-4 * SPIN * 1.5
    print(f"oracle, landing scene: touchdown at step {touch}; flying drones' |w| world vs alone, largest gap {gap:.3e} rad/s "
          f"(one-step parity bound {bound:.1e})")
    assert touch is not None and touch < 60
    assert gap > 100 * bound

"""tests/aero_ref.py -- the vectorised float64 restatement of the lifting-surface aerodynamics that tests/test_gpu_aero.py holds the
device to -- pinned without a GPU: to the reference's own numbers (tests/golden/aero.npz) at the tolerances the C oracle is held to,
and to the line-by-line oracle on the whole sweep the GPU test runs. Also here, from the reference alone: the sweep's regime census,
the share of its points that sit on a discontinuity, and the small-angle claim sincos_small rests on."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aero_ref as A  # noqa: E402
from oracle import oracle as O  # noqa: E402

dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731


def airframes():
    """(name, surface rows): the five Fixedwing surfaces, the acrowing's, the Rocket's fins."""
    out = []
    for name in ("fixedwing", "acrowing", "rocket"):
        P = O.make_params(name)
        out.append((name, P, [P.surf[s] for s in range(P.n_surf)]))
    return out


@pytest.fixture(scope="module")
def frames():
    return airframes()


def test_float64_path_reproduces_the_reference_numbers(golden_dir):
    g = np.load(os.path.join(golden_dir, "aero.npz"))
    P = O.make_params("fixedwing")
    for s in range(5):
        S = P.surf[s]
        for a, act in enumerate(g["actuations"]):
            c = np.array(A.coefficients(S, g["alphas"], float(act))).T
            np.testing.assert_allclose(c, g["coeffs"][s, a], rtol=1e-13, atol=1e-15)
        F, T = A.force_torque(S, g["vels"], float(g["force_actuation"]))
        np.testing.assert_allclose(F, g["forces"][s], rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(T, g["torques"][s], rtol=1e-12, atol=1e-13)


def test_agrees_with_the_oracle_on_the_whole_sweep(frames):
    rng = np.random.default_rng(3)
    L = O.lib()
    for name, _, surfs in frames:
        seen = []
        for S in surfs:
            key = tuple(getattr(S, f[0]) for f in O.Surface._fields_[4:]) + tuple(S.lift_unit) + tuple(S.drag_unit)
            if key in seen:  # (the Rocket's four fins differ in their position only, and pairwise in the lift unit)
                continue
            seen.append(key)
            alpha, act, V, _ = A.sweep(S)
            third = len(alpha) // len(A.SPEEDS)  # (the coefficients do not depend on the speed: one third of the sweep)
            c = np.array(A.coefficients(S, alpha[:third], act[:third]))
            ref = np.zeros((third, 3))
            for i in range(third):
                L.orc_surface_aero(C.byref(S), float(alpha[i]), float(act[i]), dp(ref[i]))
            assert np.abs(c.T - ref).max() <= 1e-12, (name, np.abs(c.T - ref).max())
            # forces: the whole sweep, every speed, a random out-of-plane component; per component |a - b| <= 1e-12 (1 + |b|)
            v = A.velocity(S, alpha, V, rng.uniform(-5.0, 5.0, len(alpha))).astype(np.float64)
            F, T = A.force_torque(S, v, act)
            Fr, Tr = np.zeros_like(F), np.zeros_like(T)
            d3 = C.c_double * 3
            va, fa, ta = v.ctypes.data, Fr.ctypes.data, Tr.ctypes.data
            force, Sp = L.orc_surface_force, C.byref(S)
            for i, a in enumerate(act.tolist()):  # (the rows in place: no array object per call)
                force(Sp, d3.from_address(va + 24 * i), a, d3.from_address(fa + 24 * i), d3.from_address(ta + 24 * i))
            eF, eT = np.abs(F - Fr) / (1.0 + np.abs(Fr)), np.abs(T - Tr) / (1.0 + np.abs(Tr))
            assert eF.max() <= 1e-12 and eT.max() <= 1e-12, (name, eF.max(), eT.max())


def test_wrench_about_base_is_torque_plus_r_cross_f(frames):
    rng = np.random.default_rng(4)
    _, _, surfs = frames[0]
    for S in surfs:
        vb, wb = rng.uniform(-20, 20, (50, 3)), rng.uniform(-3, 3, (50, 3))
        r = np.array(list(S.r))
        vloc = A.local_velocity(S, vb, wb)
        np.testing.assert_allclose(vloc, vb + np.cross(wb, r), rtol=0, atol=1e-14)
        F, T = A.force_torque(S, vloc, 0.3)
        F2, tau = A.wrench_about_base(S, vb, wb, 0.3)
        np.testing.assert_array_equal(F, F2)
        np.testing.assert_allclose(tau, T + np.cross(r, F), rtol=0, atol=1e-12)


def test_sweep_census_and_boundary_share(frames):
    """What the GPU test asserts again on the same arrays: every regime is visited, the points that sit on a jump are few."""
    for name, _, surfs in frames:
        for s, S in enumerate(surfs):
            alpha, act, V, off = A.sweep(S)
            v = A.velocity(S, alpha, V)
            counts = A.census(S, v, act)
            assert min(counts) >= 200, (name, s, dict(zip(A.CENSUS, counts)))
            al = A.angle_of_attack(S, v.astype(np.float64))
            sens, _ = A.sensitivity(S, al, act)
            jump = (sens > A.JUMP).any(0)
            share = jump.mean()
            assert share <= 0.005, (name, s, share)
            # by construction only the deliberate offset-0 points -- and the grid's own end point, pi, which is one of their centres
            stray = jump & ~(off == 0.0) & ~(alpha == np.pi)
            assert not stray.any(), (name, s, "a point off the deliberate offset-0 set sits within delta-alpha of a jump", alpha[stray], act[stray])
            print(f"{name} surface {s}: {len(alpha)} points, census {dict(zip(A.CENSUS, counts))}, boundary share {100 * share:.3f} %")
            if name == "fixedwing" and s in (0, 1):  # ailerons at actuation -1: alpha_stall_N = +0.0003 rad
                _, _, aN = A.stall_angles(S, -1.0)
                assert 0.0 < aN < 1e-3
                assert int(((act == -1.0) & (al > 0.0) & (al <= aN)).sum()) >= 3


def test_float32_restatement_is_float32_and_close(frames):
    """The E32 of the GPU test's bound: the float32 path stays in float32 and, off the jumps, within 1e-5 of the float64 one."""
    for name, _, surfs in frames[:1]:
        for S in surfs:
            alpha, act, V, _ = A.sweep(S)
            v = A.velocity(S, alpha, V)
            al = A.angle_of_attack(S, v.astype(np.float64))
            sens, _ = A.sensitivity(S, al, act)
            E, M = A.e32(S, v, act, A.regime(S, al, act), ~(sens > A.JUMP).any(0))
            assert E.max() < 1e-5 and E.min() >= 0.0, E
            print(f"{name}: E32 per output x regime\n{E}")


def test_small_angle_claim(frames):
    """uav_vehicles.hpp, lifting_surface: |a_0 + a_i| < 0.8 rad for any surface the model admits -- what licenses sincos_small, a Taylor
    pair without range reduction -- and the pair's truncation error on that range."""
    worst = 0.0
    for name, _, surfs in frames:
        for S in surfs:
            alpha = np.unique(A.sweep(S)[0])
            for act in np.linspace(-1.0, 1.0, 201):
                a0, _, _ = A.stall_angles(S, act)
                ai, _ = A.induced_angle(S, alpha, act)
                worst = max(worst, float(np.abs(a0 + ai).max()))
    print(f"max |a0 + ai| over every surface, 201 actuations, the sweep's angles: {worst:.4f} rad")
    assert worst < 0.8
    # sincos_small's two polynomials with their float32 coefficients (uav_device.hpp), against np.sin / np.cos in float64.
    # Evaluated in float64: the statement is about the polynomials -- truncation and coefficient rounding; a float32 evaluation adds
    # half an ulp of the result, 3e-8 for values in [0.5, 1), to any polynomial however exact.
    f = np.float32
    sc = [float(f(c)) for c in (-2.5052108e-8, 2.7557319e-6, -1.9841270e-4, 8.3333333e-3, -1.6666667e-1, 1.0)]
    cc = [float(f(c)) for c in (2.0876757e-9, -2.7557319e-7, 2.4801587e-5, -1.3888889e-3, 4.1666667e-2, -0.5, 1.0)]
    x = np.linspace(-0.8, 0.8, 160001)
    t = x * x
    ps = np.zeros_like(x)
    for c in sc:
        ps = ps * t + c
    pc = np.zeros_like(x)
    for c in cc:
        pc = pc * t + c
    es, ec = np.abs(x * ps - np.sin(x)).max(), np.abs(pc - np.cos(x)).max()
    # and the float32 evaluation, for the record: polynomial error plus the roundings of a float32 Horner chain
    x32 = x.astype(f)
    t32 = x32 * x32
    ps32 = np.zeros_like(x32)
    for c in sc:
        ps32 = ps32 * t32 + f(c)
    pc32 = np.zeros_like(x32)
    for c in cc:
        pc32 = pc32 * t32 + f(c)
    es32 = np.abs((x32 * ps32).astype(np.float64) - np.sin(x32.astype(np.float64))).max()
    ec32 = np.abs(pc32.astype(np.float64) - np.cos(x32.astype(np.float64))).max()
    print(f"sincos_small on [-0.8, 0.8]: polynomial error sin {es:.2e} cos {ec:.2e}; evaluated in float32 sin {es32:.2e} cos {ec32:.2e}")
    assert es < 2e-8 and ec < 2e-8
    # The float32 evaluation's own roundings on |x| <= 0.8 (t = x^2 <= 0.64), each half an ulp, on top of the polynomial's error:
    #   sin = x ps: the result (< 1: 2^-25); ps in [0.89, 1) (2^-25) times x; t's (2^-24 t) through d ps / dt = 1 / 6, times x; the
    #   product t * (-1/6 ...) in front of the last sum (< 0.125: 2^-28) times x (numpy has no fma: the device saves this one)
    #   cos = 1 + t q: the result (2^-25); q in (-0.5, -0.25) (2^-26) times t; t's (2^-24 t) times |q| <= 0.5; the product t q (< 0.5: 2^-26)
    # the steps further in are scaled by another t / 12 or less: 1e-9 for all of them.
    bs = es + 2.0 ** -25 + 0.8 * (2.0 ** -25 + 0.64 * 2.0 ** -24 / 6.0 + 2.0 ** -28) + 1e-9
    bc = ec + 2.0 ** -25 + 0.64 * 2.0 ** -26 + 0.5 * 0.64 * 2.0 ** -24 + 2.0 ** -26 + 1e-9
    print(f"  float32 bounds from the roundings: sin {bs:.2e} cos {bc:.2e}")
    assert es32 <= bs and ec32 <= bc

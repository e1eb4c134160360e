"""The attitude helpers of pyflyt_amd/csrc/uav_device.hpp on the device, routine by routine, against tests/attitude_ref.py in float64.

Every observation, cascaded controller input and body-frame velocity goes through these fp32 routines; the rest of the suite holds
them through trajectories (1e-4 .. 5e-2) and one known-answer test that stops at |pitch| = 1.5. tests/device_probes/attitude_probe.hip
calls each of them on a list of points, compiled with the product's own compiler flags. The reference is always evaluated at the
float32 inputs the device is given, and the bound is the project's (test_gpu_aero.py, test_gpu_mlp.bound_ratio):

    err <= T + M max(E32_bin, 2^-24 max|ref|_bin)

E32: the largest error of the reference formulas evaluated in numpy float32, per output and bin; T: the truncation error of a
polynomial where there is one (fp64, computed here: 2.35e-8 for fast_atan2); M = 8 for the composite functions (euler_*, canon_quat,
rot_from_quat, quat_integrate), M = 4 for the primitives (fast_atan2, fast_asin, half_angle, sincos_small, sincos_turns), whose
float32 evaluation IS the device's operation chain but for fma contraction and a 1-ulp v_rcp / v_rsq in place of a division: 4
covers those two, 8 would let a last-digit coefficient error through.

Bins: cos(pitch) for the attitude functions ([0.3, 1], [0.1, 0.3), [0.03, 0.1), [0.01, 0.03), [0.0045, 0.01), the sliver between
that and the gimbal threshold, and the gimbal branch itself: the angles lose accuracy as 1 / cos(pitch), tests/test_cpu_attitude_ref.py);
the four ranges of |result| for atan2. Angles are compared as wrapped differences. A point whose float64 sarg is within 4 x 2^-24 of
0.99999 is on a jump: it must match the reference of one side, with all outputs on that side. A canonical quaternion whose roll or yaw
(half the yaw in the gimbal branch: it is 2 atan2) lies within its bound of +-pi may match -ref; everywhere else the sign must match."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attitude_ref as R  # noqa: E402
from __graft_entry__ import HIPCC_FLAGS  # noqa: E402  (-ffp-contract=off and the scheduler switches decide the bits)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
(ROT, MUL, EULER, EULER_FAST, QUAT, CANON, HALF, HALF_QUAT, ATAN2, ATAN2_X2, ASIN, SINCOS_SMALL, SINCOS_TURNS, SINCOS_ANGLE, INTEGRATE) = range(15)
EPS = R.EPS
M_COMPOSITE, M_PRIMITIVE = 8.0, 4.0
f32, f64 = np.float32, np.float64
HALF_PI32 = f32(0.5) * R.PI32


# ------------------------------------------------------------------------------------------------ the probe
class Probe:
    def __init__(self, lib):
        self.lib = lib
        fp = C.POINTER(C.c_float)
        lib.attitude_probe.argtypes = [C.c_int, fp, C.c_size_t, fp, C.c_size_t, C.c_int]
        lib.attitude_probe.restype = C.c_int
        lib.attitude_probe_strides.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.attitude_probe_strides.restype = C.c_int

    def run(self, which, inp):
        a, b = C.c_int(), C.c_int()
        assert self.lib.attitude_probe_strides(which, C.byref(a), C.byref(b)) == 0
        inp = np.ascontiguousarray(inp, f32)
        if inp.ndim == 1:
            inp = inp[:, None]
        assert inp.ndim == 2 and inp.shape[1] == a.value, (inp.shape, a.value)
        out = np.empty((len(inp), b.value), f32)
        fp = C.POINTER(C.c_float)
        rc = self.lib.attitude_probe(which, inp.ctypes.data_as(fp), inp.size, out.ctypes.data_as(fp), out.size, len(inp))
        assert rc == 0, f"attitude_probe({which}): status {rc}"
        assert np.isfinite(out).all(), f"routine {which}: non-finite output, first at point {np.argwhere(~np.isfinite(out))[0]}, input {inp[np.argwhere(~np.isfinite(out))[0][0]]}"
        return out


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    so = tmp_path_factory.mktemp("probe") / "libattitudeprobe.so"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", *HIPCC_FLAGS, "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "device_probes", "attitude_probe.hip"), "-o", str(so)])
    return Probe(C.CDLL(str(so)))


class World:
    """Built once per module: the attitude points (unit, then the two scalings of the Haar set), their tables, the device's outputs."""

    def __init__(self, probe):
        self.probe = probe
        self.att = R.Attitudes()
        self.q = self.att.all_points()
        self.tab = R.AttitudeTables(self.q)
        self.T_atan = R.atan_truncation()
        self.euler = probe.run(EULER, self.q)
        self.euler_fast = probe.run(EULER_FAST, self.q)
        self.canon = probe.run(CANON, self.q)


@pytest.fixture(scope="module")
def world(probe):
    return World(probe)


RATIOS = {}


def record(routine, output, bin_name, ratio):
    if np.size(ratio):
        k = (routine, output, bin_name)
        RATIOS[k] = max(RATIOS.get(k, 0.0), float(np.max(ratio)))


def print_ratios(title):
    print(f"\n{title}: worst err / bound per routine, output and bin")
    for routine in dict.fromkeys(k[0] for k in RATIOS):
        outs = dict.fromkeys(k[1] for k in RATIOS if k[0] == routine)
        for o in outs:
            print(f"  {routine:22s} {o:10s} " + "  ".join(f"{k[2]} {v:.2f}" for k, v in RATIOS.items() if k[0] == routine and k[1] == o))
    RATIOS.clear()


def held(routine, outputs, err, bnd, bins, names, where=None):
    """err, bnd: (N, K); records the worst ratio per output and bin and asserts every one <= 1."""
    err, bnd = np.atleast_2d(err.T).T, np.atleast_2d(bnd.T).T
    ratio = err / np.maximum(bnd, 1e-300)
    where = np.ones(len(err), bool) if where is None else where
    for b, name in enumerate(names):
        m = where & (bins == b)
        for k, o in enumerate(outputs):
            record(routine, o, name, ratio[m, k])
    bad = where & (ratio > 1.0).any(1)
    if bad.any():
        i = int(np.argmax(np.where(where, ratio.max(1), 0.0)))
        raise AssertionError(f"{routine}: {int(bad.sum())} of {int(where.sum())} points over the bound; worst err / bound {ratio[i]} at point {i} (bin {names[bins[i]]}): err {err[i]}, bound {bnd[i]}")


# ------------------------------------------------------------------------------------------------ (a) fast_atan2, fast_asin
@pytest.mark.gpu
def test_fast_atan2_and_fast_asin(probe, world):
    y, x = R.atan2_points()
    ref = np.arctan2(y.astype(f64), x.astype(f64))
    bins = R.atan_bins(ref)
    E = R.per_bin_max(np.abs(R.fast_atan2_f32(y, x).astype(f64) - ref), bins, 4)
    B = R.bound(world.T_atan, M_PRIMITIVE, E, R.per_bin_max(np.abs(ref), bins, 4))
    got = probe.run(ATAN2, np.stack([y, x], 1))[:, 0]
    err = np.abs(got.astype(f64) - ref)
    print(f"\nfast_atan2 on {len(y)} points: E32 per bin " + ", ".join(f"{e:.2e}" for e in E) + "; bound " + ", ".join(f"{b:.2e}" for b in B)
          + "; device max error per bin " + ", ".join(f"{e:.2e}" for e in R.per_bin_max(err, bins, 4)))
    print(f"  the figure the comment stated (1.2e-7) holds: {bool(err.max() <= 1.2e-7)}; in the first octant: {bool(err[bins == 0].max() <= 1.2e-7)}")
    held("fast_atan2", ("r",), err, B[bins], bins, R.ATAN_BIN_NAMES)
    assert (np.signbit(got) == np.signbit(y)).all()  # copysign(r, y), zeros included
    # signed zeros and axes, to the bit
    cases = [((0.0, 0.0), 0.0), ((-0.0, 0.0), -0.0), ((0.0, -1.0), R.PI32), ((-0.0, -1.0), -R.PI32), ((1.0, 0.0), HALF_PI32), ((-1.0, 0.0), -HALF_PI32),
             ((1.0, -0.0), HALF_PI32), ((-1.0, -0.0), -HALF_PI32), ((0.0, 1.0), 0.0), ((-0.0, 1.0), -0.0), ((0.0, 3e9), 0.0), ((-2e-9, 0.0), -HALF_PI32)]
    pts = np.array([c[0] for c in cases] * 6, f32)[:64]  # (a whole wave)
    want = np.array([c[1] for c in cases] * 6, f32)[:64]
    out = probe.run(ATAN2, pts)[:, 0]
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), [(tuple(p), float(o), float(w)) for p, o, w in zip(pts, out, want) if o.tobytes() != w.tobytes()]
    # exact diagonals: +-pi/4, +-3pi/4 under the bound (they are in the sweep too; here by name)
    d = np.array([[sy * m, sx * m] for m in (1e-18, 0.3, 1.0, 777.0, 1e18) for sy in (1, -1) for sx in (1, -1)], f32)
    dref = np.arctan2(d[:, 0].astype(f64), d[:, 1].astype(f64))
    assert np.allclose(np.abs(dref) % (np.pi / 2), np.pi / 4, atol=1e-15)
    assert (np.abs(probe.run(ATAN2, d)[:, 0] - dref) <= B[R.atan_bins(dref)]).all()

    xs = R.asin_points()
    aref = np.arcsin(xs.astype(f64))
    abins = R.atan_bins(aref)
    Ea = R.per_bin_max(np.abs(R.fast_asin_f32(xs).astype(f64) - aref), abins, 4)
    Ba = R.bound(world.T_atan, M_PRIMITIVE, Ea, R.per_bin_max(np.abs(aref), abins, 4))
    ga = probe.run(ASIN, xs)[:, 0]
    held("fast_asin", ("r",), np.abs(ga.astype(f64) - aref), Ba[abins], abins, R.ATAN_BIN_NAMES)
    assert ga[xs == 1.0][0] == HALF_PI32 and ga[xs == -1.0][0] == -HALF_PI32 and ga[xs == 0.0][0] == 0.0
    print(f"  fast_asin on {len(xs)} points: E32 " + ", ".join(f"{e:.2e}" for e in Ea[:2]) + "; device max error " + f"{np.abs(ga - aref).max():.2e}")
    print_ratios("fast_atan2, fast_asin")


# ------------------------------------------------------------------------------------------------ (b) fast_atan2_x2 == fast_atan2
@pytest.mark.gpu
def test_fast_atan2_x2_is_fast_atan2_bit_for_bit(probe):
    """uav_device.hpp: "each element rounds as the scalar instruction does, so both results equal fast_atan2's bit for bit"."""
    y, x = R.atan2_points()
    one = probe.run(ATAN2, np.stack([y, x], 1))[:, 0].view(np.uint32)
    perm = np.random.default_rng(5).permutation(len(y))  # a different point in the other element
    assert (perm != np.arange(len(y))).mean() > 0.99
    two = probe.run(ATAN2_X2, np.stack([y, x, y[perm], x[perm]], 1)).view(np.uint32)
    assert np.array_equal(two[:, 0], one) and np.array_equal(two[:, 1], one[perm]), (int((two[:, 0] != one).sum()), int((two[:, 1] != one[perm]).sum()))
    swp = probe.run(ATAN2_X2, np.stack([y[perm], x[perm], y, x], 1)).view(np.uint32)
    assert np.array_equal(swp[:, 1], one) and np.array_equal(swp[:, 0], one[perm]), (int((swp[:, 1] != one).sum()), int((swp[:, 0] != one[perm]).sum()))


# ------------------------------------------------------------------------------------------------ (c) sincos_small, sincos_turns, the wrapper
@pytest.mark.gpu
def test_sincos_small_turns_and_the_dogfight_wrapper(probe):
    def run(name, which, x, angle, chain, T, bins, names, stated):
        s, c = chain(x)
        ref = np.stack([np.sin(angle), np.cos(angle)], 1)
        E = R.per_bin_max(np.abs(np.stack([s, c], 1).astype(f64) - ref), bins, len(names))
        B = R.bound(T, M_PRIMITIVE, E, 1.0)  # max|ref| = 1 in every bin
        got = probe.run(which, x).astype(f64)
        err = np.abs(got - ref)
        held(name, ("sin", "cos"), err, B[bins], bins, names)
        print(f"  {name}: E32 {E.max(0)}; bound {B.max(0)}; device max error {err.max(0)}; the stated {stated:.0e} holds: {bool(err.max() <= stated)}")
        return got, err

    print()
    x = R.small_points()
    bins = (np.abs(x) > f32(0.8)).astype(int)
    T = np.array([R.sincos_truncation(0.8), R.sincos_truncation(1.0)])
    _, err = run("sincos_small", SINCOS_SMALL, x, x.astype(f64), R.sincos_small_f32, T, bins, ("|x| <= 0.8", "0.8 < |x| <= 1"), 1e-7)
    print(f"    on [-0.8, 0.8] the stated 8e-8 holds: {bool(err[bins == 0].max() <= 8e-8)} ({err[bins == 0].max():.2e})")
    # sincos_turns: |r| <= pi/4 after the reduction, the polynomials' error there
    Tt = np.array(R.sincos_truncation(np.pi / 4 * (1 + 1e-6)))
    u = R.turn_points()
    zb = np.zeros(len(u), int)
    got, _ = run("sincos_turns", SINCOS_TURNS, u, 2.0 * np.pi * u.astype(f64), R.sincos_turns_f32, Tt[None, :], zb, ("[0, 1]",), 1e-7)
    for uu, (s, c) in ((0.0, (0, 1)), (0.25, (1, 0)), (0.5, (0, -1)), (0.75, (-1, 0)), (1.0, (0, 1))):  # the values float32 has exactly
        m = u == f32(uu)
        assert m.any() and (got[m, 0] == s).all() and (got[m, 1] == c).all(), (uu, got[m])
    for k in (1, 3, 5, 7):  # the odd eighths: sqrt(1/2), under the bound (checked with the rest); both outputs equal in size to within it
        m = u == f32(k / 8.0)
        assert m.any() and np.abs(np.abs(got[m]) - np.sqrt(0.5)).max() <= 4 * EPS + Tt.max()
    a = R.angle_points()
    got, _ = run("sincos_angle (dogfight)", SINCOS_ANGLE, a, a.astype(f64), R.sincos_angle_f32, Tt[None, :], np.zeros(len(a), int), ("[-pi, pi]",), 1e-7)
    assert (got[a == 0.0] == np.array([0.0, 1.0])).all()
    print_ratios("sincos_small, sincos_turns, dogfight.hpp's sincos_angle")


# ------------------------------------------------------------------------------------------------ (d) half_angle, quat_from_half_angles, quat_from_euler
@pytest.mark.gpu
def test_half_angle(probe):
    """"no trig, no cancellation": the error stays at a few 2^-24 over the whole circle, c = -1 included."""
    c, s = R.half_angle_points()
    rc, rs = R.half_angle(c.astype(f64), s.astype(f64))
    ref = np.stack([rc, rs], 1)
    ch, sh = R.half_angle_f32(c, s)
    # bins: the two selects (c >= 0, c < 0)
    bins = (c < 0).astype(int)
    E = R.per_bin_max(np.abs(np.stack([ch, sh], 1).astype(f64) - ref), bins, 2)
    B = R.bound(0.0, M_PRIMITIVE, E, 1.0)
    got = probe.run(HALF, np.stack([c, s], 1))
    assert (got[:, 0] >= 0).all() and not np.signbit(got[:, 0]).any()                      # cos(t/2) >= 0 on (-pi, pi]
    assert (np.signbit(got[:, 1]) == np.signbit(s)).all()                                  # sin(t/2) has the sign of sin t, zeros included
    held("half_angle", ("ch", "sh"), np.abs(got.astype(f64) - ref), B[bins], bins, ("c >= 0", "c < 0"))
    edge = got[-6:]
    assert np.array_equal(edge, np.array([[1, 0], [1, -0.0], [0, 1], [0, -1], [np.sqrt(0.5), np.sqrt(0.5)], [np.sqrt(0.5), -np.sqrt(0.5)]], f32)), edge
    print(f"\nhalf_angle: E32 {E.max(0)}, bound {B.max(0)}")
    print_ratios("half_angle")


@pytest.mark.gpu
def test_quat_from_half_angles_and_quat_from_euler(probe, world):
    rng = np.random.default_rng(9)
    n = 4096
    e = np.concatenate([rng.uniform(-np.pi, np.pi, (n, 3)), world.tab.euler[: world.att.n]]).astype(f32)
    h = 0.5 * e.astype(f64)
    x = np.stack([np.cos(h[:, 0]), np.sin(h[:, 0]), np.cos(h[:, 1]), np.sin(h[:, 1]), np.cos(h[:, 2]), np.sin(h[:, 2])], 1).astype(f32)
    cr, sr, cp, sp, cy, sy = x.astype(f64).T
    ref = np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy], 1)
    a, b, c, d, g, k = x.T
    r32 = np.stack([b * c * g - a * d * k, a * d * g + b * c * k, a * c * k - b * d * g, a * c * g + b * d * k], 1)  # the same products in float32
    zb = np.zeros(len(x), int)
    E = R.per_bin_max(np.abs(r32.astype(f64) - ref), zb, 1)
    held("quat_from_half_angles", "xyzw", np.abs(probe.run(HALF_QUAT, x).astype(f64) - ref), R.bound(0.0, M_PRIMITIVE, E, 1.0)[zb], zb, ("all",))
    qref = R.quat_from_euler(e.astype(f64))
    Eq = R.per_bin_max(np.abs(R.quat_from_euler(e, f32).astype(f64) - qref), zb, 1)
    got = probe.run(QUAT, e)
    held("quat_from_euler", "xyzw", np.abs(got.astype(f64) - qref), R.bound(0.0, M_COMPOSITE, Eq, 1.0)[zb], zb, ("all",))
    assert np.abs(np.linalg.norm(got.astype(f64), axis=1) - 1.0).max() <= 2e-7
    print_ratios("quat_from_half_angles, quat_from_euler")


# ------------------------------------------------------------------------------------------------ (e) euler_from_quat, euler_from_quat_fast, canon_quat
def is_gimbal(e):
    """The branch a device output took: the gimbal branch returns roll = 0 and pitch = +-(0.5f * kPi) exactly."""
    return (e[:, 0] == 0.0) & (np.abs(e[:, 1]) == HALF_PI32)


def euler_bounds(world, fast):
    tab = world.tab
    T = np.zeros((R.N_BINS, 3))
    if fast:
        T[:] = world.T_atan           # fast_atan2, and fast_asin through it
        T[R.GIMBAL_BIN, 2] *= 2.0     # the gimbal yaw is 2 fast_atan2
    return R.bound(T, M_COMPOSITE, tab.e_euler, tab.m_euler)


def check_euler(world, name, got, fast):
    tab = world.tab
    B = euler_bounds(world, fast)
    got = got.astype(f64)
    smooth = ~tab.jump
    err = np.abs(R.wrap(got - tab.euler))
    held(name, ("roll", "pitch", "yaw"), err, B[tab.bins], tab.bins, R.BIN_NAMES, where=smooth)
    # on a jump: one side or the other, all three angles on the same side
    j = np.flatnonzero(tab.jump)
    on_s = (np.abs(R.wrap(got[j] - tab.smooth[j])) <= B[0]).all(1)
    on_g = (np.abs(R.wrap(got[j] - tab.gimbal[j])) <= B[R.GIMBAL_BIN]).all(1)
    assert (on_s | on_g).all(), (name, "a point on the jump matches neither side", world.q[j[~(on_s | on_g)][0]], got[j[~(on_s | on_g)][0]])
    return len(j), int(on_s.sum()), int(on_g.sum())


def canon_bounds(world):
    return R.bound(0.0, M_COMPOSITE, world.tab.e_canon, world.tab.m_canon)


def canon_err(world, got, side):
    """|got - ref| per component against one side's canonical quaternion ("own": the float64 branch), -ref admitted where an atan2
    of the reference lies within its bound of +-pi (roll, yaw; half the gimbal yaw), and only there."""
    tab = world.tab
    Be = euler_bounds(world, True)
    e = {"own": tab.euler, "smooth": tab.smooth, "gimbal": tab.gimbal}[side]
    c = {"own": tab.canon, "smooth": tab.canon_smooth, "gimbal": tab.canon_gimbal}[side]
    b = {"own": tab.bins, "smooth": np.where(tab.bins == R.GIMBAL_BIN, 0, tab.bins), "gimbal": np.full(len(e), R.GIMBAL_BIN)}[side]
    gim = b == R.GIMBAL_BIN
    near = np.where(gim, np.abs(e[:, 2]) / 2 >= np.pi - Be[b, 2] / 2, (np.abs(e[:, 0]) >= np.pi - Be[b, 0]) | (np.abs(e[:, 2]) >= np.pi - Be[b, 2]))
    got = got.astype(f64)
    plus, minus = np.abs(got - c), np.abs(got + c)
    flip = near & (minus.max(1) < plus.max(1))
    return np.where(flip[:, None], minus, plus), b, near


@pytest.mark.gpu
def test_euler_and_canon_on_every_attitude_point(world):
    tab, att = world.tab, world.att
    print(f"\n{len(world.q)} points ({att.n} unit, {len(world.q) - att.n} scaled by 0.5 and 1.37); on a jump {int(tab.jump.sum())}")
    for name, got, fast in (("euler_from_quat", world.euler, False), ("euler_from_quat_fast", world.euler_fast, True)):
        nj, ns, ng = check_euler(world, name, got, fast)
        print(f"  {name}: of {nj} points on the jump {ns} match the smooth side, {ng} the gimbal side")
    # the two forms take the same branch as each other, and as the reference, wherever the point is not on the jump
    smooth = ~tab.jump
    g0, g1 = is_gimbal(world.euler), is_gimbal(world.euler_fast)
    assert (g0 == g1)[smooth].all(), world.q[smooth & (g0 != g1)][:4]
    assert (g0 == (tab.bins == R.GIMBAL_BIN))[smooth].all(), world.q[smooth & (g0 != (tab.bins == R.GIMBAL_BIN))][:4]
    assert g0[tab.bins == R.GIMBAL_BIN].sum() >= 128
    # canon_quat
    Bc = canon_bounds(world)
    err, b, near = canon_err(world, world.canon, "own")
    held("canon_quat", "xyzw", err, Bc[b], b, R.BIN_NAMES, where=smooth)
    j = np.flatnonzero(tab.jump)
    es, bs, _ = canon_err(world, world.canon, "smooth")
    eg, bg, _ = canon_err(world, world.canon, "gimbal")
    ok = (es[j] <= Bc[bs[j]]).all(1) | (eg[j] <= Bc[bg[j]]).all(1)
    assert ok.all(), ("canon_quat: a point on the jump matches neither side", world.q[j[~ok][0]], world.canon[j[~ok][0]])
    assert np.abs(np.linalg.norm(world.canon.astype(f64), axis=1) - 1.0).max() <= 2e-7
    print(f"  canon_quat: {int(near.sum())} points within the bound of an atan2 of +-pi (either sign admitted)")
    # non-unit inputs give the unit input's result: x 0.5 is exact in float32, so the SAME reference point
    h = att.family["haar"]
    n_h = h.stop - h.start
    half = slice(att.n, att.n + n_h)
    B = euler_bounds(world, True)
    for name, got in (("euler_from_quat", world.euler), ("euler_from_quat_fast", world.euler_fast)):
        assert np.array_equal(tab.euler[h], tab.euler[half])
        assert (np.abs(R.wrap(got[half].astype(f64) - tab.euler[h])) <= B[tab.bins[h]]).all(), name
    # x 1.37 rounds each component anew: the unit input's result to within the bound of both
    big = slice(att.n + n_h, att.n + 2 * n_h)
    for got, Bx, wrapd in ((world.euler, B, True), (world.euler_fast, B, True), (world.canon, Bc, False)):
        d = got[big].astype(f64) - got[h].astype(f64)
        d = np.abs(R.wrap(d)) if wrapd else np.minimum(np.abs(d), np.abs(got[big].astype(f64) + got[h].astype(f64)))
        assert (d <= Bx[tab.bins[h]] + Bx[tab.bins[big]]).all()
    print_ratios("euler_from_quat, euler_from_quat_fast, canon_quat")
    print("  E32 of the Euler angles per bin (roll / pitch / yaw): " + "; ".join(f"{n} " + "/".join(f"{x:.1e}" for x in e) for n, e in zip(R.BIN_NAMES, tab.e_euler)))
    print("  E32 of canon per bin (largest component): " + "; ".join(f"{n} {e.max():.1e}" for n, e in zip(R.BIN_NAMES, tab.e_canon)))


# ------------------------------------------------------------------------------------------------ (f) canon_quat against its definition
@pytest.mark.gpu
def test_canon_quat_against_the_composition_of_its_definition(probe, world):
    """canon_quat is quat_from_euler(euler_from_quat(q)): by those very two calls in the gimbal branch -- bit for bit -- and by half-angle
    algebra elsewhere -- under the bound."""
    tab = world.tab
    composed = probe.run(QUAT, world.euler)
    gim = (tab.bins == R.GIMBAL_BIN) & ~tab.jump
    assert gim.sum() >= 128
    a, b = world.canon[gim].view(np.uint32), composed[gim].view(np.uint32)
    assert np.array_equal(a, b), (int((a != b).any(1).sum()), "gimbal-branch points differ from quat_from_euler(euler_from_quat(q))")
    Bc = canon_bounds(world)
    rest = ~(tab.bins == R.GIMBAL_BIN) & ~tab.jump
    _, bb, near = canon_err(world, world.canon, "own")
    d = np.abs(world.canon.astype(f64) - composed)
    d = np.where(near[:, None], np.minimum(d, np.abs(world.canon.astype(f64) + composed)), d)
    held("canon_quat - composed", "xyzw", d, Bc[bb], bb, R.BIN_NAMES, where=rest)
    print_ratios("canon_quat against quat_from_euler(euler_from_quat(q)) from the probe's own kernels")


# ------------------------------------------------------------------------------------------------ (g) rot_from_quat, mul, mulT
@pytest.mark.gpu
def test_rot_from_quat_mul_mulT(probe, world):
    tab, att = world.tab, world.att
    BR = R.bound(0.0, M_COMPOSITE, tab.e_R, tab.m_R)          # per bin and entry
    got = probe.run(ROT, world.q).astype(f64)
    held("rot_from_quat", ("entry",) * 9, np.abs(got - tab.R), BR[tab.bins], tab.bins, R.BIN_NAMES)
    # R R^T - I: with R = R0 + E, R0 orthogonal, |E_ik| <= b: (R R^T - I)_ij = sum_k E_ik R0_jk + R0_ik E_jk + E_ik E_jk
    #   <= b (sum_k |R0_jk| + |R0_ik|) + 3 b^2, from the reference's own entries
    b = BR[tab.bins].max(1)
    G = got.reshape(-1, 3, 3)
    A0 = np.abs(tab.R.reshape(-1, 3, 3)).sum(2)  # (N, 3): sum_k |R0_ik|
    orth = np.abs(G @ G.transpose(0, 2, 1) - np.eye(3))
    obound = b[:, None, None] * (A0[:, :, None] + A0[:, None, :]) + 3.0 * (b * b)[:, None, None]
    held("rot_from_quat", ("R R^T - I",), (orth / obound).max((1, 2)), np.ones(len(b)), tab.bins, R.BIN_NAMES)
    # scaled quaternions give the same R: x 0.5 against the unit point's reference, x 1.37 against the unit point's output
    h = att.family["haar"]
    n_h = h.stop - h.start
    half, big = slice(att.n, att.n + n_h), slice(att.n + n_h, att.n + 2 * n_h)
    assert (np.abs(got[half] - tab.R[h]) <= BR[tab.bins[h]]).all()
    assert (np.abs(got[big] - got[h]) <= BR[tab.bins[h]] + BR[tab.bins[big]]).all()
    # mul, mulT on the unit points with velocities of a few m/s. Per component, with |R_ij| <= 1 and v1 = |v|_1:
    #   R v: the entries' error b v1, and three roundings of an fma chain whose partial sums stay under v1: 3 x 2^-24 v1
    #   R^T (R v) - v: the first product's error e1 passes through R^T (at most sum_i e1_i = 3 e1), the second product adds its
    #   own b |u|_1 + 3 x 2^-24 |u|_1 with |u|_1 <= sqrt(3) |v|_2 <= sqrt(3) v1
    rng = np.random.default_rng(12)
    qn = world.q[: att.n]
    v = rng.uniform(-8.0, 8.0, (att.n, 3)).astype(f32)
    out = probe.run(MUL, np.concatenate([qn, v], 1)).astype(f64)
    R0 = tab.R[: att.n].reshape(-1, 3, 3)
    v64 = v.astype(f64)
    v1 = np.abs(v64).sum(1)
    bn = b[: att.n]
    e1 = (bn + 3 * EPS) * v1
    bins = tab.bins[: att.n]
    held("mul", "xyz", np.abs(out[:, 0:3] - np.einsum("nij,nj->ni", R0, v64)), np.repeat(e1[:, None], 3, 1), bins, R.BIN_NAMES)
    held("mulT", "xyz", np.abs(out[:, 3:6] - np.einsum("nji,nj->ni", R0, v64)), np.repeat(e1[:, None], 3, 1), bins, R.BIN_NAMES)
    e2 = 3 * e1 + (bn + 3 * EPS) * np.sqrt(3.0) * v1
    held("mulT(R, mul(R, v)) - v", "xyz", np.abs(out[:, 6:9] - v64), np.repeat(e2[:, None], 3, 1), bins, R.BIN_NAMES)
    print_ratios("rot_from_quat, mul, mulT")
    print("  E32 of rot_from_quat per bin (largest entry): " + "; ".join(f"{n} {e.max():.1e}" for n, e in zip(R.BIN_NAMES, tab.e_R)))


# ------------------------------------------------------------------------------------------------ (h) quat_integrate
@pytest.mark.gpu
def test_quat_integrate_against_the_exponential_map(probe, world):
    q, w = R.integration_points(world.att)
    hd = f32(R.HALF_DT)
    ref = R.exp_map_step(q, w, f64(hd))
    th = np.linalg.norm(w.astype(f64), axis=1) * f64(hd)
    # abi_env.hpp refuses a context whose sqrt(3) max_coord_vel dt / 2 exceeds pi/8: the clamp corners lie inside the polynomials' range
    assert (th[:R.N_CORNERS] <= np.pi / 8).all() and (np.abs(w[:R.N_CORNERS]) == 100.0).all() and th.max() <= np.pi / 8
    zb = np.zeros(len(q), int)
    E = R.per_bin_max(np.abs(R.exp_map_step(q, w, hd, f32).astype(f64) - ref), zb, 1)
    T = sum(R.integrate_truncation())  # the sinc polynomial's error scales the vector part (|.| <= 1), the cosine's the scalar one
    B = R.bound(T, M_COMPOSITE, E, 1.0)
    got = probe.run(INTEGRATE, np.concatenate([q, w, np.full((len(q), 1), hd, f32)], 1))
    held("quat_integrate", "xyzw", np.abs(got.astype(f64) - ref), B[zb], zb, ("all",))
    assert np.abs(np.linalg.norm(got.astype(f64), axis=1) - 1.0).max() <= 2e-7  # the figure of test_gpu_kat.py
    z = slice(R.N_CORNERS, R.N_CORNERS + R.N_ZERO)
    assert not w[z].any()
    qz = q[z].astype(f64)
    assert (np.abs(got[z] - qz / np.linalg.norm(qz, axis=1, keepdims=True)) <= B[0]).all()  # w = 0: q, normalised
    print(f"\nquat_integrate: E32 {E[0]}, T {T:.1e}, bound {B[0]}; | |q| - 1 | <= {np.abs(np.linalg.norm(got.astype(f64), axis=1) - 1.0).max():.2e}")
    print_ratios("quat_integrate")


# ------------------------------------------------------------------------------------------------ (i) a lane does not depend on its wave
@pytest.mark.gpu
def test_a_lane_does_not_depend_on_its_wave(probe, world):
    """euler_from_quat_fast and canon_quat branch on the gimbal test per lane: the same points in waves none of whose lanes takes the
    gimbal branch, in waves of gimbal points only, interleaved, and with one gimbal lane among 63 others, bit for bit (the arrangements
    of test_gpu_aero.py::test_a_lane_does_not_depend_on_its_wave)."""
    tab = world.tab
    unit = np.arange(len(world.q)) < world.att.n
    il = np.flatnonzero(unit & (tab.bins != R.GIMBAL_BIN) & (tab.bins != 0) & ~tab.jump)
    ig = np.flatnonzero(unit & (tab.bins == R.GIMBAL_BIN) & ~tab.jump)
    assert len(il) >= 1024 and len(ig) >= 128, (len(il), len(ig))
    il = il[np.linspace(0, len(il) - 1, 1024).astype(int)]  # (spread over the families: Haar, the ladder, the special angles)
    ig = np.resize(ig, 1024)
    mixed = np.empty(2048, int); mixed[0::2] = il; mixed[1::2] = ig
    lone = np.concatenate([ig[:16, None], np.tile(il[:63], 16).reshape(16, 63)], 1).ravel()
    x = world.q

    def same(a, b, what):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, int((a.view(np.uint32) != b.view(np.uint32)).sum()))

    for which, name, whole in ((EULER_FAST, "euler_from_quat_fast", world.euler_fast), (CANON, "canon_quat", world.canon), (EULER, "euler_from_quat", world.euler)):
        calm, full = probe.run(which, x[il]), probe.run(which, x[ig])
        mix, one = probe.run(which, x[mixed]), probe.run(which, x[lone])
        if which != CANON:  # (the arrangements are what they say: no lane of the calm waves takes the gimbal branch, every lane of the full ones does)
            assert not is_gimbal(calm).any() and is_gimbal(full).all()
        same(calm, mix[0::2], name + ": smooth points, alone and interleaved with gimbal ones")
        same(full, mix[1::2], name + ": gimbal points, alone and interleaved with smooth ones")
        same(full[:16], one[0::64], name + ": a gimbal point among 63 smooth ones")
        same(calm[:63], one[1:64], name + ": smooth points next to one gimbal lane")
        same(calm, whole[il], name + ": the same points in the order of the whole set")

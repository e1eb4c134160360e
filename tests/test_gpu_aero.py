"""The lifting-surface aerodynamics on the device, form by form, against tests/aero_ref.py in float64.

The device has four hand-written forms of lifting_surfaces.py:266-498 -- lifting_surface() (uav_vehicles.hpp: the generic Fixedwing
vehicle, the Rocket's fins), FwHot::surface<LIFT_Y>, FwHot::surface_pair (packed fp32, scheduled by hand) and FwHot::surface_pair_x2
(fixedwing_fast.hpp) -- that the rest of the suite holds through trajectories only. tests/device_probes/aero_probe.hip calls each of
them on a list of points, compiled with the product's own compiler flags; here the points are a dense sweep of the angle of attack
with deliberate points at and around every stall angle, +-pi/2, 0 and the branch cut, and the bound is derived per point:

    err <= sens + 8 max(E32, 2^-24 max|ref|)

sens: what DELTA_ALPHA = 4e-7 rad of angle error (aero_ref.py) does to the coefficient, from the float64 reference; E32: the largest
error of the reference evaluated in float32, per output and regime (the convention of test_gpu_mlp.bound_ratio). A point within
DELTA_ALPHA of a jump of the coefficient must match the reference on one of its two sides instead. Forces and torques get the same
bound carried through QA, the chord and the arm (Ref.__init__ writes the propagation out)."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aero_ref as A  # noqa: E402
from __graft_entry__ import HIPCC_FLAGS  # noqa: E402  (-ffp-contract=off and the scheduler switches decide the bits)
from oracle import oracle as O  # noqa: E402
from pyflyt_amd import _lib as L  # noqa: E402
from pyflyt_amd import build_params  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERIC, SCALAR, PAIR, X2, ACCUMULATE = range(5)
PAIR_IDS = ((0, 1), (2, 4))  # FwTable.pair: (left aileron, right aileron), (horizontal tail, main wing)
EPS = 2.0 ** -24
MARGIN = 8.0
f32 = np.float32


# ------------------------------------------------------------------------------------------------ the probe
class Probe:
    def __init__(self, lib):
        self.lib = lib
        fp = C.POINTER(C.c_float)
        lib.aero_probe.argtypes = [C.POINTER(L.PfParams), C.c_size_t, C.c_int, C.c_int, fp, C.c_size_t, fp, C.c_size_t, C.c_int]
        lib.aero_probe.restype = C.c_int
        lib.aero_probe_table.argtypes = [C.POINTER(L.PfParams), C.c_size_t, fp, C.c_size_t]
        lib.aero_probe_table.restype = C.c_int
        lib.aero_probe_strides.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.aero_probe_strides.restype = C.c_int

    def status(self, P, impl, sel, inp):
        a, b = C.c_int(), C.c_int()
        assert self.lib.aero_probe_strides(impl, C.byref(a), C.byref(b)) == 0
        inp = np.ascontiguousarray(inp, f32)
        assert inp.ndim == 2 and inp.shape[1] == a.value, (inp.shape, a.value)
        out = np.empty((len(inp), b.value), f32)
        fp = C.POINTER(C.c_float)
        rc = self.lib.aero_probe(C.byref(P), C.sizeof(P), impl, sel, inp.ctypes.data_as(fp), inp.size, out.ctypes.data_as(fp), out.size, len(inp))
        return rc, out

    def run(self, P, impl, sel, inp):
        rc, out = self.status(P, impl, sel, inp)
        assert rc == 0, f"aero_probe: status {rc}"
        assert np.isfinite(out).all(), f"non-finite output, first at point {np.argwhere(~np.isfinite(out))[0]}"
        return out

    def table(self, P):
        self.lib.aero_probe_table_bytes.restype = C.c_size_t
        t = np.zeros(self.lib.aero_probe_table_bytes() // 4, f32)
        assert t.size == 112  # two FwSurf2, FwSurf, FwBody: the layout test_fw_table_from_params reads the rows from
        ok = self.lib.aero_probe_table(C.byref(P), C.sizeof(P), t.ctypes.data_as(C.POINTER(C.c_float)), t.nbytes)
        assert ok in (0, 1), ok
        return bool(ok), t


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    so = tmp_path_factory.mktemp("probe") / "libaeroprobe.so"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", *HIPCC_FLAGS, "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "device_probes", "aero_probe.hip"), "-o", str(so)])
    return Probe(C.CDLL(str(so)))


# ------------------------------------------------------------------------------------------------ airframes, points, references
class Frame:
    def __init__(self, name, P, Q):
        self.name, self.P, self.Q = name, P, Q
        self.n = Q.n_surf
        self.surfs = [Q.surf[s] for s in range(self.n)]
        self.r32 = [np.array(list(P.surf[s].r), f32).astype(np.float64) for s in range(self.n)]
        self.fast = name != "rocket"
        self.E = {}  # surface -> (E32, max|ref|), from the coefficient sweep


class Points:
    """Body velocity per lift axis, angular velocity, actuation. The out-of-plane component lies along the surface's torque unit."""

    def __init__(self, alpha, act, V, oop=None, wb=None, off=None):
        self.alpha, self.act, self.V = (np.asarray(x, np.float64) for x in (alpha, act, V))
        self.act = self.act.astype(f32).astype(np.float64)  # (the reference is evaluated at the inputs the device is given)
        self.n = len(self.alpha)
        self.oop = np.zeros(self.n) if oop is None else oop
        self.wb = np.zeros((self.n, 3), f32) if wb is None else np.asarray(wb, f32)
        self.off = np.full(self.n, np.nan) if off is None else off
        self._vb = {}

    def vb(self, S):
        key = tuple(S.lift_unit) + tuple(S.drag_unit)
        if key not in self._vb:
            self._vb[key] = A.velocity(S, self.alpha, self.V, self.oop)
        return self._vb[key]

    def inputs(self, S, per_point=1):
        a = np.repeat(self.act.astype(f32)[:, None], per_point, 1)
        return np.concatenate([self.vb(S), self.wb, a, a], 1)  # cmd == a: the lag is the identity


def abs_cross(r, b):
    """|r| x |b| with every term added: what a bound b on a force does to r x f."""
    r = np.abs(r)
    return np.stack([r[1] * b[:, 2] + r[2] * b[:, 1], r[2] * b[:, 0] + r[0] * b[:, 2], r[0] * b[:, 1] + r[1] * b[:, 0]], 1)


class Ref:
    """One surface on one set of points: the float64 reference at the inputs the device is given, and the bound, point by point."""

    def __init__(self, frame, s, pts, extra_delta=0.0, input_rel=0.0):
        S = self.S = frame.surfs[s]
        self.frame, self.s = frame, s
        K = A._K(S, np.float64)
        self.K = K
        vb, wb = pts.vb(S).astype(np.float64), pts.wb.astype(np.float64)
        self.act = pts.act
        self.vloc = A.local_velocity(S, vb, wb)
        la, fa = self.vloc @ K.lift, self.vloc @ K.drag
        self.h, self.speed = np.hypot(la, fa), np.sqrt((self.vloc ** 2).sum(1))
        self.ca, self.sa = fa / self.h, -la / self.h
        self.QA = K.half_rho * self.speed ** 2 * K.area
        self.alpha = A.angle_of_attack(S, self.vloc)
        # What the device's local velocity may be off by: nothing where wb = 0 (vb + 0 x r is exact), else the float32 roundings of
        # vb + wb x r, 2^-23 (|vb| + |wb||r|) per component (test (g) checks that figure); input_rel: a relative error of the inputs
        # themselves (a reference computed at velocities that were rounded to float32 afterwards).
        wn = np.sqrt((wb ** 2).sum(1))
        dv = np.where(wn > 0, 2.0 ** -23 * (np.sqrt((vb ** 2).sum(1)) + wn * np.linalg.norm(K.r)), 0.0) + input_rel * self.speed
        # -> the angle: both in-plane components off by dv turn (fa, la) by at most sqrt(2) dv / h
        self.delta = A.DELTA_ALPHA + np.sqrt(2.0) * dv / self.h + extra_delta
        # -> QA = hra (vx^2 + vy^2 + vz^2): relative 2 sqrt(3) dv / |v|. Zero where the velocity is exact (wb = 0, no input_rel): the
        # float32 roundings of QA itself are part of E32, which runs force_torque in float32 and divides by the float64 QA.
        self.relqa = 2.0 * np.sqrt(3.0) * dv / self.speed
        self.c = np.array(A.coefficients(S, self.alpha, self.act))
        self.reg = A.regime(S, self.alpha, self.act)
        side = lambda k: np.array(A.coefficients(S, A.wrap(self.alpha + k * self.delta), self.act))  # noqa: E731
        self.cm, self.cp, cm3, cp3 = side(-1), side(1), side(-3), side(3)
        self.sens = np.maximum(np.abs(self.cm - self.c), np.abs(self.cp - self.c))
        self.flag = (self.sens > A.JUMP).any(0)
        if s not in frame.E:  # (the first Ref of a surface is its coefficient sweep)
            frame.E[s] = A.e32(S, pts.vb(S), self.act, self.reg, ~self.flag)
        E, M = frame.E[s]
        # (c) coefficients: sens + 8 max(E32, 2^-24 max|ref|); where the velocity itself is uncertain, QA's share of that (the
        # recovered coefficient divides by the exact QA)
        self.b = A.coefficient_bound(self.sens, E, M, self.reg, MARGIN) + self.relqa * np.abs(self.c)
        # a point on a jump: the reference delta to either side, with the smooth bound of that side (the coefficient's change over the
        # next 2 delta for sens: the device's own angle lies within delta of the point, on that side)
        self.bm = A.coefficient_bound(np.abs(cm3 - self.cm), E, M, A.regime(S, A.wrap(self.alpha - self.delta), self.act), MARGIN) + self.relqa * np.abs(self.cm)
        self.bp = A.coefficient_bound(np.abs(cp3 - self.cp), E, M, A.regime(S, A.wrap(self.alpha + self.delta), self.act), MARGIN) + self.relqa * np.abs(self.cp)
        # forces over QA: fn = Cl ca + Cd sa, fp = Cl sa - Cd ca, linear in the coefficients; F = lift fn + forward fp
        bn = np.abs(self.ca) * self.b[0] + np.abs(self.sa) * self.b[1]
        bq = np.abs(self.sa) * self.b[0] + np.abs(self.ca) * self.b[1]
        self.bF = np.abs(K.lift)[None, :] * bn[:, None] + np.abs(K.drag)[None, :] * bq[:, None]
        # torque over QA: T = CM chord torque_unit; about the base tau = T + r x F: the arm times the force's bound, and the float32
        # roundings of the device's own r x f + t chain (four per component, each half an ulp of a term)
        self.bT = np.abs(K.torque)[None, :] * (K.chord * self.b[2])[:, None]
        self.F, self.T = A.force_torque(S, self.vloc, self.act)
        self.tau = self.T + np.cross(K.r, self.F)
        chain = 4 * EPS * (abs_cross(K.r, np.abs(self.F)) + np.abs(self.T)) / self.QA[:, None]
        self.btau = self.bT + abs_cross(K.r, self.bF) + chain
        # a moment coefficient taken back out of tau with the device's OWN force and float32 r (the fast forms return rz fp - rx fn
        # + tm): the force's error cancels, what is left is the roundings of that chain, over the chord
        self.cm_slack = (chain @ np.abs(K.torque)) / K.chord


RATIOS = {}


def check(ref, impl, F, T=None, tau=None, what="sweep"):
    """Device force F (N, 3), link torque T or torque about the base tau (NaN where the form does not return the component), all in
    the body frame, against ref: the recovered coefficients under bound (c), either side at a jump; then force and torque over QA."""
    K, r32 = ref.K, ref.frame.r32[ref.s]
    F = np.asarray(F, np.float64)
    slack = np.zeros_like(ref.c)
    if T is None:
        tau = np.asarray(tau, np.float64)
        T = np.nan_to_num(tau) - np.cross(r32, F)
        T = np.where(np.isnan(tau), 0.0, T)
        slack[2] = ref.cm_slack
    T = np.asarray(T, np.float64)
    rec = A.recover(ref.S, ref.vloc, F, T)
    err = np.abs(rec - ref.c)
    smooth = ~ref.flag
    ratio = err / (ref.b + slack)
    key = f"{ref.frame.name} s{ref.s} {impl}"
    for o, oname in enumerate(("Cl", "Cd", "CM")):
        for k in range(5):
            m = smooth & (ref.reg == k)
            if m.any():
                RATIOS[(key, oname, k)] = max(RATIOS.get((key, oname, k), 0.0), float(ratio[o, m].max()))
    bad = smooth & (ratio > 1.0).any(0)
    if bad.any():
        i = np.argmax(np.where(smooth, ratio.max(0), 0.0))
        raise AssertionError(f"{key} ({what}): {int(bad.sum())} of {int(smooth.sum())} smooth points over the bound; worst ratio {ratio[:, i]} at alpha {ref.alpha[i]:.7f} "
                             f"act {ref.act[i]} regime {A.REGIMES[ref.reg[i]]}: got {rec[:, i]}, reference {ref.c[:, i]}, bound {ref.b[:, i] + slack[:, i]}")
    if ref.flag.any():  # on a jump: the reference at alpha - delta OR at alpha + delta, all three outputs on the same side
        f = ref.flag
        on_m = (np.abs(rec - ref.cm)[:, f] <= (ref.bm + slack)[:, f]).all(0)
        on_p = (np.abs(rec - ref.cp)[:, f] <= (ref.bp + slack)[:, f]).all(0)
        if not (on_m | on_p).all():
            i = np.flatnonzero(f)[np.argmin(on_m | on_p)]
            raise AssertionError(f"{key} ({what}): a point on a jump matches neither side: alpha {ref.alpha[i]:.7f} act {ref.act[i]}: got {rec[:, i]}, "
                                 f"below {ref.cm[:, i]}, above {ref.cp[:, i]}")
    # forces and torques over QA, smooth points
    q = ref.QA[:, None]
    eF = np.abs(F - ref.F) / q
    assert (eF <= ref.bF)[smooth].all(), (key, what, "force", float((eF / np.maximum(ref.bF, 1e-300))[smooth].max()))
    if tau is None:
        eT = np.abs(T - ref.T) / q
        assert (eT <= ref.bT)[smooth].all(), (key, what, "torque", float((eT / np.maximum(ref.bT, 1e-300))[smooth].max()))
    else:
        eT = np.where(np.isnan(tau), 0.0, np.abs(np.nan_to_num(tau) - ref.tau) / q)
        assert (eT <= ref.btau)[smooth].all(), (key, what, "torque about the base", float((eT / np.maximum(ref.btau, 1e-300))[smooth].max()))


def print_ratios(title):
    print(f"\n{title}: worst err / bound per implementation, output and regime (regimes: {', '.join(A.REGIMES)})")
    keys = sorted({k[0] for k in RATIOS})
    for key in keys:
        print(f"  {key:28s} " + "  ".join(f"{o} " + "/".join(f"{RATIOS.get((key, o, k), 0.0):.2f}" for k in range(5)) for o in ("Cl", "Cd", "CM")))


def pair_half(out, e, base=0):
    """(F, tau, a') of one half of a FwPairOut block: fp along +x, fn along +z, ty the y component of the torque about the base."""
    fp, fn, ty, a = (out[:, base + 2 * j + e].astype(np.float64) for j in range(4))
    z, nan = np.zeros_like(fp), np.full_like(fp, np.nan)
    return np.stack([fp, z, fn], 1), np.stack([nan, ty, nan], 1), a


def evaluate(probe, frame, pts, impls=(GENERIC, SCALAR, PAIR, X2, ACCUMULATE)):
    """Every implementation on pts, one launch each: {(impl name, surface): dict(F, T or tau, a, raw)}."""
    res = {}
    lz = frame.surfs[0]
    for s in range(frame.n):
        if GENERIC in impls:
            o = probe.run(frame.P, GENERIC, s, pts.inputs(frame.surfs[s]))
            res[("generic", s)] = dict(F=o[:, 0:3], T=o[:, 3:6], tau=o[:, 9:12], vloc=o[:, 6:9], a=o[:, 12], raw=o)
        if frame.fast and SCALAR in impls:
            o = probe.run(frame.P, SCALAR, s, pts.inputs(frame.surfs[s]))
            res[("scalar", s)] = dict(F=o[:, 0:3], tau=o[:, 3:6].astype(np.float64), a=o[:, 6], raw=o)
    if frame.fast:
        for k, ids in enumerate(PAIR_IDS):
            if PAIR in impls:
                o = probe.run(frame.P, PAIR, k, pts.inputs(lz, 2))
                for e, s in enumerate(ids):
                    F, tau, a = pair_half(o, e)
                    res[("pair", s)] = dict(F=F, tau=tau, a=a, raw=o)
            if ACCUMULATE in impls:
                o = probe.run(frame.P, ACCUMULATE, k, pts.inputs(lz, 2))
                for e, s in enumerate(ids):
                    res[("accumulate", s)] = dict(F=o[:, 6 * e:6 * e + 3], tau=o[:, 6 * e + 3:6 * e + 6].astype(np.float64), raw=o)
        if X2 in impls:
            o = probe.run(frame.P, X2, 0, pts.inputs(lz, 4))
            for k, ids in enumerate(PAIR_IDS):
                for e, s in enumerate(ids):
                    F, tau, a = pair_half(o, e, 8 * k)
                    res[("x2", s)] = dict(F=F, tau=tau, a=a, raw=o)
    return res


def check_all(frame, refs, res, what):
    for (impl, s), d in res.items():
        if impl == "generic":
            check(refs[s], impl, d["F"], T=d["T"], what=what)
            check(refs[s], impl + " r x f", d["F"], tau=d["tau"].astype(np.float64), what=what)
        else:
            check(refs[s], impl, d["F"], tau=d["tau"], what=what)


class World:
    """Built once per module: airframes, the sweep of each, its references, and the device's outputs on it."""

    def __init__(self, probe):
        self.probe = probe
        self.frames = {
            "fixedwing": Frame("fixedwing", build_params("fixedwing", "none"), O.make_params("fixedwing")),
            "acrowing": Frame("acrowing", build_params("fixedwing", "none", vehicle_options=dict(drone_model="acrowing")), O.make_params("acrowing")),
            "rocket": Frame("rocket", build_params("rocket", "none"), O.make_params("rocket")),
        }
        self.sweep, self.refs, self.out = {}, {}, {}
        for name, fr in self.frames.items():
            parts, seen = [], set()
            for S in fr.surfs:  # the union of the surfaces' sweeps: every surface meets every other one's deliberate points too
                p = A.sweep(S)
                if p[0].tobytes() not in seen:
                    seen.add(p[0].tobytes())
                    parts.append(p)
            al, ac, V, off = (np.concatenate([p[j] for p in parts]) for j in range(4))
            self.sweep[name] = Points(al, ac, V, off=off)
            self.refs[name] = [Ref(fr, s, self.sweep[name]) for s in range(fr.n)]
            self.out[name] = evaluate(probe, fr, self.sweep[name])


@pytest.fixture(scope="module")
def world(probe):
    return World(probe)


# ------------------------------------------------------------------------------------------------ census
@pytest.mark.gpu
def test_regime_census_and_boundary_share(world):
    for name, fr in world.frames.items():
        pts = world.sweep[name]
        for s, ref in enumerate(world.refs[name]):
            counts = A.census(ref.S, pts.vb(ref.S), pts.act)
            assert min(counts) >= 200, (name, s, dict(zip(A.CENSUS, counts)))
            share = ref.flag.mean()
            assert share <= 0.005, (name, s, share)
            print(f"{name} surface {s}: {pts.n} points, census " + ", ".join(f"{c} {k}" for c, k in zip(counts, A.CENSUS)) + f"; on a jump {100 * share:.3f} %")
    for s in (0, 1):  # the ailerons at actuation -1: alpha_stall_N = +0.0003 rad, 0 < alpha <= aN is positive stall at the clamped end
        ref = world.refs["fixedwing"][s]
        _, _, aN = A.stall_angles(ref.S, -1.0)
        m = (ref.act == -1.0) & (ref.alpha > 0.0) & (ref.alpha <= aN)
        assert 0.0 < aN < 1e-3 and int(m.sum()) >= 3, (aN, int(m.sum()))
        assert (ref.reg[m] == A.POS_STALL).all()


# ------------------------------------------------------------------------------------------------ (b) the dense sweep, (d) no NaN
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["fixedwing", "acrowing", "rocket"])
def test_dense_sweep_against_float64(world, name):
    RATIOS.clear()
    check_all(world.frames[name], world.refs[name], world.out[name], "dense sweep")  # (Probe.run has asserted every output finite)
    print_ratios(f"{name}, dense sweep, {world.sweep[name].n} points")
    fr = world.frames[name]
    for s in range(fr.n):
        E, M = fr.E[s]
        print(f"  surface {s}: E32 x 1e7 per regime  Cl " + "/".join(f"{x:.1f}" for x in E[0] * 1e7) + "  Cd " + "/".join(f"{x:.1f}" for x in E[1] * 1e7)
              + "  CM " + "/".join(f"{x:.1f}" for x in E[2] * 1e7))


# ------------------------------------------------------------------------------------------------ (a) the reference's own numbers
@pytest.mark.gpu
def test_reference_numbers_on_every_implementation(world, golden_dir):
    g = np.load(os.path.join(golden_dir, "aero.npz"))
    fr = world.frames["fixedwing"]
    RATIOS.clear()
    # coefficients: aero.npz's (surface, actuation, alpha) grid at every speed of the sweep
    al = np.tile(np.tile(g["alphas"], len(g["actuations"])), len(A.SPEEDS))
    ac = np.tile(np.repeat(g["actuations"], len(g["alphas"])), len(A.SPEEDS))
    V = np.repeat(A.SPEEDS, len(g["alphas"]) * len(g["actuations"]))
    pts = Points(al, ac, V)
    res = evaluate(world.probe, fr, pts)
    refs = []
    for s in range(5):
        alpha_dev = A.angle_of_attack(fr.surfs[s], pts.vb(fr.surfs[s]).astype(np.float64))
        # (the float32 velocity's angle is not aero.npz's alpha to the last bit: the difference joins delta-alpha)
        ref = Ref(fr, s, pts, extra_delta=np.abs(A.wrap(alpha_dev - al)))
        gold = np.tile(g["coeffs"][s].reshape(-1, 3), (len(A.SPEEDS), 1)).T
        own = np.array(A.coefficients(ref.S, al, ac))
        assert np.abs(own - gold).max() < 1e-13  # (test_cpu_aero_ref, again: the reference IS aero.npz here)
        ref.c = np.where(ref.flag, ref.c, gold)
        refs.append(ref)
    check_all(fr, refs, res, "aero.npz coefficients")
    # forces: aero.npz's velocities at actuation 0.3. The file's forces are those of the float64 velocities; the device gets them
    # rounded to float32: a relative input error of 2^-24 per component.
    vels = g["vels"]
    for axis_of, sids in (("z", (0, 1, 2, 4)), ("y", (3,))):
        S0 = fr.surfs[sids[0]]
        K = A._K(S0, np.float64)
        la, fa, oop = vels @ K.lift, vels @ K.drag, vels @ K.torque
        pv = Points(np.arctan2(-la, fa), np.full(len(vels), float(g["force_actuation"])), np.hypot(la, fa), oop=oop)
        assert np.abs(pv.vb(S0) - vels).max() <= 2 * EPS * np.abs(vels).max()
        impls = (GENERIC, SCALAR) if axis_of == "y" else (GENERIC, SCALAR, PAIR, X2, ACCUMULATE)
        rs = evaluate(world.probe, fr, pv, impls)
        for s in sids:
            ref = Ref(fr, s, pv, input_rel=2 * EPS)
            assert np.abs(ref.F - g["forces"][s]).max() <= 1e-5 * np.abs(g["forces"][s]).max()  # (same points up to the rounding of the input)
            ref.F, ref.T = g["forces"][s], g["torques"][s]
            ref.tau = ref.T + np.cross(ref.K.r, ref.F)
            ref.c = A.recover(ref.S, vels, ref.F, ref.T)
            for (impl, ss), d in rs.items():
                if ss != s:
                    continue
                if impl == "generic":
                    check(ref, impl, d["F"], T=d["T"], what="aero.npz forces")
                else:
                    check(ref, impl, d["F"], tau=d["tau"], what="aero.npz forces")
    print_ratios("fixedwing, aero.npz's coefficients and forces")


# ------------------------------------------------------------------------------------------------ (b) wb != 0, (g) local velocity
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["fixedwing", "acrowing", "rocket"])
def test_forces_and_torques_about_the_base_with_rotation(world, name):
    fr = world.frames[name]
    sw = world.sweep[name]
    rng = np.random.default_rng(17)
    idx = np.arange(rng.integers(0, 5), sw.n, 5)
    n = len(idx)
    wb = rng.normal(size=(n, 3))
    wb *= (rng.uniform(0.0, 6.0, n) / np.linalg.norm(wb, axis=1))[:, None]  # |wb| <= 6 rad/s
    pts = Points(sw.alpha[idx], sw.act[idx], sw.V[idx], oop=rng.uniform(-1.0, 1.0, n) * sw.V[idx], wb=wb)
    res = evaluate(world.probe, fr, pts)
    refs = [Ref(fr, s, pts) for s in range(fr.n)]
    RATIOS.clear()
    check_all(fr, refs, res, "random out-of-plane velocity and rotation")
    print_ratios(f"{name}, rotating, {n} points")
    worst = 0.0
    # (g) vb + wb x r against local_velocity at 2^-23 (|vb| + |wb||r|). The bound is one for the arithmetic (a product, an fma and a
    # sum: half an ulp each), so the reference takes the link position the device is given, the float32 one: with the float64 r of
    # the model file the Rocket's upper fins (r = (+-0.35, 0, 2.051) m, |wb||r| up to 12 m/s next to 1 m/s) measured 1.31 of the bound, on r's rounding
    # (0.97 with the device's own r; the aeroplanes 0.73).
    for s in range(fr.n):
        S = fr.surfs[s]
        vb, w = pts.vb(S).astype(np.float64), pts.wb.astype(np.float64)
        tol = 2.0 ** -23 * (np.linalg.norm(vb, axis=1) + np.linalg.norm(w, axis=1) * np.linalg.norm(list(S.r)))
        e = np.abs(res[("generic", s)]["vloc"] - A.local_velocity(S, vb, w, r=fr.r32[s])).max(1)
        worst = max(worst, float((e / tol).max()))
        assert (e <= tol).all(), (name, s, float((e / tol).max()))
    print(f"  local velocity: worst error / (2^-23 (|vb| + |wb||r|)) = {worst:.3f}")


# ------------------------------------------------------------------------------------------------ (d) degenerate inputs
@pytest.mark.gpu
def test_degenerate_inputs(world):
    probe = world.probe
    for name, fr in world.frames.items():
        # V = 0: forces and torques exactly 0
        n = 64
        z = Points(np.zeros(n), np.linspace(-1, 1, n), np.zeros(n))
        for (impl, s), d in evaluate(probe, fr, z).items():
            assert not np.asarray(d["F"]).any(), (name, impl, s, "force at V = 0")
            for k in ("T", "tau"):
                if k in d:
                    assert not np.nan_to_num(np.asarray(d[k], np.float64)).any(), (name, impl, s, k, "at V = 0")
        # fa = 0 exactly with la != 0: alpha = +-pi/2; la = +-0 with fa < 0: the branch cut, either side; 300 m/s
        for S in {tuple(S.lift_unit): S for S in fr.surfs}.values():
            K = A._K(S, np.float64)
            acts = np.array(A.ACTUATIONS)
            vs = []
            for la, fa in ((10.0, 0.0), (-10.0, 0.0), (-0.0, -10.0), (0.0, -10.0), (1.0, 0.0), (-40.0, 0.0)):
                vs.append(np.array(fa) * K.drag + np.array(la) * K.lift)
            edge = np.repeat(np.array(vs), len(acts), 0)
            sids = [s for s in range(fr.n) if tuple(fr.surfs[s].lift_unit) == tuple(S.lift_unit)]
            p = Points(np.zeros(len(edge)), np.tile(acts, len(vs)), np.ones(len(edge)))
            p._vb[tuple(S.lift_unit) + tuple(S.drag_unit)] = edge.astype(f32)
            assert (np.abs(A.angle_of_attack(S, edge[: 2 * len(acts)])) == np.pi / 2).all()
            # (alpha = atan2(-la, fa): la = -0.0 is the UPPER side of the cut for the function, +pi, and la = +0.0 the lower one; but
            #  the sign of a zero does not survive the dot product with the lift unit, here or in the generic form: either side)
            assert np.arctan2(0.0, -10.0) == np.pi and np.arctan2(-0.0, -10.0) == -np.pi
            fast_impls = (GENERIC, SCALAR) if tuple(S.lift_unit) == (0.0, 1.0, 0.0) and fr.fast else (GENERIC, SCALAR, PAIR, X2, ACCUMULATE)
            res = {k: v for k, v in evaluate(probe, fr, p, fast_impls).items() if k[1] in sids}
            check_all(fr, {s: Ref(fr, s, p) for s in sids}, res, "fa = 0, la = +-0")
            al = np.tile(np.linspace(-np.pi, np.pi, 129)[1:], len(acts))
            fastp = Points(al, np.repeat(acts, 128), np.full(len(al), 300.0))
            res = {k: v for k, v in evaluate(probe, fr, fastp, fast_impls).items() if k[1] in sids}
            check_all(fr, {s: Ref(fr, s, fastp) for s in sids}, res, "300 m/s")


# ------------------------------------------------------------------------------------------------ (e) a lane does not depend on its wave
def _settled(ref, margin=1e-3):
    """Points whose regime is the same margin either side: the device cannot classify them differently from the reference."""
    S = ref.S
    return (A.regime(S, A.wrap(ref.alpha - margin), ref.act) == ref.reg) & (A.regime(S, A.wrap(ref.alpha + margin), ref.act) == ref.reg) & ~ref.flag


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["fixedwing", "acrowing"])
def test_a_lane_does_not_depend_on_its_wave(world, name):
    """surface<>, surface_pair and surface_pair_x2 skip the post-stall code in a wave none of whose lanes is stalled (__any(!linear)):
    the same points in waves that skip it and in waves that run it, bit for bit."""
    fr, sw, refs, probe = world.frames[name], world.sweep[name], world.refs[name], world.probe
    lin = [_settled(r) & (r.reg == A.LINEAR) for r in refs]
    stl = [_settled(r) & (r.reg != A.LINEAR) for r in refs]

    def arrangements(lin_m, stall_m, S, per_point):
        il, ist = np.flatnonzero(lin_m), np.flatnonzero(stall_m)
        assert len(il) >= 1024 and len(ist) >= 1024, (len(il), len(ist))
        il = il[np.linspace(0, len(il) - 1, 1024).astype(int)]     # (spread over the actuations and speeds)
        ist = ist[np.linspace(0, len(ist) - 1, 1024).astype(int)]  # (and over the stalled regimes)
        x = sw.inputs(S, per_point)
        mixed = np.empty(2048, int); mixed[0::2] = il; mixed[1::2] = ist          # branch taken, every wave half linear
        lone = np.tile(il[:63], 16).reshape(16, 63); lone = np.concatenate([ist[:16, None], lone], 1).ravel()  # one stalled lane among 63 linear
        return x, il, ist, mixed, lone

    def same(a, b, what):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, what, int((a.view(np.uint32) != b.view(np.uint32)).sum()))

    def run_all(impl, sel, S, lin_m, stall_m, per_point, what):
        x, il, ist, mixed, lone = arrangements(lin_m, stall_m, S, per_point)
        calm = probe.run(fr.P, impl, sel, x[il])       # waves that are all linear: the branch is skipped
        full = probe.run(fr.P, impl, sel, x[ist])      # waves of stalled points
        mix = probe.run(fr.P, impl, sel, x[mixed])
        one = probe.run(fr.P, impl, sel, x[lone])
        same(calm, mix[0::2], what + ": linear points, alone and interleaved with stalled ones")
        same(full, mix[1::2], what + ": stalled points, alone and interleaved with linear ones")
        same(full[:16], one[0::64], what + ": a stalled point among 63 linear ones")
        same(calm[:63], one[1:64], what + ": linear points next to one stalled lane")

    for s in range(5):
        run_all(SCALAR, s, fr.surfs[s], lin[s], stl[s], 1, f"surface<> on surface {s}")
    lz = fr.surfs[0]
    for k, (a, b) in enumerate(PAIR_IDS):  # a wave is calm when BOTH halves are linear in every lane; stalled: either half
        run_all(PAIR, k, lz, lin[a] & lin[b], (stl[a] | stl[b]) & (_settled(refs[a]) & _settled(refs[b])), 2, f"surface_pair on pair {k}")
    all_lin = lin[0] & lin[1] & lin[2] & lin[4]
    any_stl = (stl[0] | stl[1] | stl[2] | stl[4]) & _settled(refs[0]) & _settled(refs[1]) & _settled(refs[2]) & _settled(refs[4])
    run_all(X2, 0, lz, all_lin, any_stl, 4, "surface_pair_x2")


# ------------------------------------------------------------------------------------------------ (f) the statements in the comments
def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def assert_the_fast_forms_are_one(name, scalar, pair, x2, acc):
    """scalar: {surface: raw surface<false> rows}; pair, acc: {pair index: raw rows}; x2: raw rows -- all on the same points.
    Every comparison is of bits, none exempted. surface<false> and accumulate() ADD fp, fn and the y torque to totals that start at
    +0.0, so the pair's raw outputs are compared as 0 + x, the operation both of them apply (it turns a -0.0 into +0.0)."""
    for k, ids in enumerate(PAIR_IDS):  # fixedwing_fast.hpp, surface_pair_x2: "bit-identical results", updated actuations included
        pr = pair[k]
        assert np.array_equal(_bits(x2[:, 8 * k:8 * k + 8]), _bits(pr)), (name, k, int((_bits(x2[:, 8 * k:8 * k + 8]) != _bits(pr)).sum()))
        # surface_pair: "surface<false> element by element (same operations on each element)": fp, fn, the y torque about the base, a'
        for e, s in enumerate(ids):
            sc = scalar[s]
            for col, what in ((0, "fp"), (2, "fn"), (4, "tau.y"), (6, "a'")):
                a, b = sc[:, col], pr[:, col + e] if what == "a'" else pr[:, col + e] + f32(0.0)
                d = _bits(a) != _bits(b)
                assert not d.any(), (name, f"surface {s} {what}: {int(d.sum())} points differ, largest {np.abs(a.astype(np.float64) - b)[d].max():.3e}")
            # accumulate() on the pair's outputs is the tail of surface<false>: the whole F and tau
            d = _bits(acc[k][:, 6 * e:6 * e + 6]) != _bits(sc[:, :6])
            assert not d.any(), (name, s, "accumulate", int(d.sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["fixedwing", "acrowing"])
def test_x2_is_pair_and_pair_is_surface_bit_for_bit(world, name):
    out = world.out[name]
    assert_the_fast_forms_are_one(name, {s: out[("scalar", s)]["raw"] for s in (0, 1, 2, 4)}, {k: out[("pair", ids[0])]["raw"] for k, ids in enumerate(PAIR_IDS)},
                                  out[("x2", 0)]["raw"], {k: out[("accumulate", ids[0])]["raw"] for k, ids in enumerate(PAIR_IDS)})


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["fixedwing", "acrowing"])
def test_each_half_has_its_own_actuation(world, name):
    """Everywhere else both halves of a pair, and all four surfaces of x2, get the same actuation, and the ailerons are the same row
    twice: an x / y mix-up of a, defl, a0, aP or aN inside the packed forms would go unseen. Here every surface draws its own
    actuation of the sweep's seven, and each half must still be surface<false> at ITS actuation, bit for bit, and
    the float64 reference at it under bound (c)."""
    fr, sw, probe = world.frames[name], world.sweep[name], world.probe
    rng = np.random.default_rng(29)
    idx = np.arange(rng.integers(0, 4), sw.n, 4)
    n = len(idx)
    lz = fr.surfs[0]
    base = Points(sw.alpha[idx], sw.act[idx], sw.V[idx])
    vb, wb = base.vb(lz), base.wb
    order = (0, 1, 2, 4)
    a = rng.choice(np.array(A.ACTUATIONS, f32), (n, 4))
    a[np.arange(n), rng.integers(0, 4, n)] = sw.act[idx].astype(f32)  # (one surface per point stays on its deliberate stall-angle points)
    cmd = a  # (the lag is the identity: test_actuator_lag has distinct (a, cmd) per half; the reference takes a few distinct actuations)
    scalar = {s: probe.run(fr.P, SCALAR, s, np.concatenate([vb, wb, a[:, j:j + 1], cmd[:, j:j + 1]], 1)) for j, s in enumerate(order)}
    pair = {k: probe.run(fr.P, PAIR, k, np.concatenate([vb, wb, a[:, 2 * k:2 * k + 2], cmd[:, 2 * k:2 * k + 2]], 1)) for k in range(2)}
    acc = {k: probe.run(fr.P, ACCUMULATE, k, np.concatenate([vb, wb, a[:, 2 * k:2 * k + 2], cmd[:, 2 * k:2 * k + 2]], 1)) for k in range(2)}
    x2 = probe.run(fr.P, X2, 0, np.concatenate([vb, wb, a, cmd], 1))
    assert_the_fast_forms_are_one(name, scalar, pair, x2, acc)
    assert len({tuple(r) for r in a[:64]}) > 32 and (a[:, 0] != a[:, 1]).mean() > 0.5 and (a[:, 2] != a[:, 3]).mean() > 0.5
    RATIOS.clear()
    for k, ids in enumerate(PAIR_IDS):
        for e, s in enumerate(ids):
            p = Points(sw.alpha[idx], a[:, 2 * k + e], sw.V[idx])
            F, tau, _ = pair_half(pair[k], e)
            check(Ref(fr, s, p), "pair, own actuation", F, tau=tau, what="independent actuations")
            F, tau, _ = pair_half(x2, e, 8 * k)
            check(Ref(fr, s, p), "x2, own actuation", F, tau=tau, what="independent actuations")
    print_ratios(f"{name}, an actuation per surface, {n} points")


# ------------------------------------------------------------------------------------------------ (g) the actuator lag
@pytest.mark.gpu
def test_actuator_lag(world):
    fr, probe = world.frames["fixedwing"], world.probe
    rng = np.random.default_rng(23)
    n = 4096
    a, cmd = rng.uniform(-1, 1, (n, 4)).astype(f32), rng.uniform(-1, 1, (n, 4)).astype(f32)
    cmd[: n // 4] = a[: n // 4]  # cmd == a leaves a unchanged to the bit
    vb = np.tile(np.array([[12.0, 0.5, -1.0]], f32), (n, 1))
    wb = np.zeros((n, 3), f32)
    dt = fr.Q.world.dt

    def held(new, col, s, what):
        tau = fr.surfs[s].tau
        ref = a[:, col].astype(np.float64) + (dt / tau) * (cmd[:, col].astype(np.float64) - a[:, col])
        # a' = fma(dt_tau, cmd - a, a): the difference's rounding and dt_tau's own (each half an ulp, times dt_tau |cmd - a|), the result's
        tol = EPS * (np.abs(ref) + 2.0 * (dt / tau) * np.abs(cmd[:, col].astype(np.float64) - a[:, col])) + 1e-45
        assert (np.abs(new - ref) <= tol).all(), (what, s, float((np.abs(new - ref) / tol).max()))
        q = n // 4
        assert np.array_equal(np.ascontiguousarray(new[:q], f32).view(np.uint32), a[:q, col].copy().view(np.uint32)), (what, s)

    for s in range(5):
        x = np.concatenate([vb, wb, a[:, :1], cmd[:, :1]], 1)
        held(probe.run(fr.P, GENERIC, s, x)[:, 12], 0, s, "generic")
        held(probe.run(fr.P, SCALAR, s, x)[:, 6], 0, s, "scalar")  # (the line in front of surface<true> in both ticks, through its formula)
    for k, ids in enumerate(PAIR_IDS):
        o = probe.run(fr.P, PAIR, k, np.concatenate([vb, wb, a[:, :2], cmd[:, :2]], 1))
        for e, s in enumerate(ids):
            held(o[:, 6 + e], e, s, "pair")
    o = probe.run(fr.P, X2, 0, np.concatenate([vb, wb, a, cmd], 1))
    for k, ids in enumerate(PAIR_IDS):
        for e, s in enumerate(ids):
            held(o[:, 8 * k + 6 + e], 2 * k + e, s, "x2")


# ------------------------------------------------------------------------------------------------ (h) fw_table_from_params
@pytest.mark.gpu
def test_fw_table_from_params(world):
    probe = world.probe
    for name in ("fixedwing", "acrowing"):
        P = world.frames[name].P
        ok, t = probe.table(P)
        assert ok
        rows = {}
        fields = ("rx", "ry", "rz", "cl3d", "a0b", "aPb", "aNb", "tau_eta", "c1", "ipa", "exp_term", "cd0", "defl_lim", "dt_tau", "hra", "chord")
        for k, ids in enumerate(PAIR_IDS):  # FwSurf2: sixteen (first, second) pairs
            blk = t[32 * k:32 * k + 32].reshape(16, 2)
            for e, s in enumerate(ids):
                rows[s] = dict(zip(fields, blk[:, e]))
        rows[3] = dict(zip(fields, t[64:80]))
        for s in range(5):
            S, R = P.surf[s], rows[s]
            want = dict(rx=S.r[0], ry=S.r[1], rz=S.r[2], cl3d=S.Cl_alpha_3D, a0b=S.alpha_0_base, aPb=S.alpha_stall_P_base, aNb=S.alpha_stall_N_base,
                        tau_eta=S.aero_tau_eta, c1=f32(f32(S.flap_to_chord) - f32(1.0)) * f32(S.aero_tau_eta), ipa=S.inv_pi_aspect, exp_term=S.exp_term,
                        cd0=S.Cd_0, defl_lim=S.deflection_limit_rad, dt_tau=S.dt_over_tau, hra=S.half_rho_area, chord=S.chord)
            for f in fields:
                assert f32(R[f]) == f32(want[f]), (name, s, f, R[f], want[f])
    # configurations the fast path does not take: the table is refused, and the probe launches none of the fast forms on it
    P = world.frames["fixedwing"].P
    for field, value in (("ticks_per_control", 4), ("flight_mode", 1), ("n_motors", 2)):
        Q = L.PfParams.from_buffer_copy(P)
        setattr(Q, field, value)
        assert probe.table(Q)[0] is False, field
        rc, _ = probe.status(Q, PAIR, 0, np.zeros((64, 10), f32))
        assert rc == -4, (field, rc)
    Q = L.PfParams.from_buffer_copy(P)
    Q.surf[2].lift[1], Q.surf[2].lift[2] = 1.0, 0.0  # a horizontal tail that lifts along +y
    assert probe.table(Q)[0] is False
    assert probe.table(world.frames["rocket"].P)[0] is False

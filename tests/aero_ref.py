"""TEST INFRASTRUCTURE: the lifting-surface aerodynamics (abstractions/lifting_surfaces.py:266-498 of the reference) as plain vectorised
numpy -- np.arctan2, np.sin, np.cos, np.interp, no kernel tricks -- in float64, or with every constant, input and operation in float32
(`dtype=np.float32`: what rounding the formulas in single precision costs, the E32 of tests/test_gpu_aero.py's bound).

`S` is a row of oracle.make_params(...).surf. tests/test_cpu_aero_ref.py pins the float64 path to tests/golden/aero.npz (the
reference's own numbers) and to the line-by-line C oracle; tests/test_gpu_aero.py holds the device's four forms against it."""
import numpy as np

LINEAR, POS_STALL, POS_BEYOND, NEG_STALL, NEG_BEYOND = range(5)
REGIMES = ("linear", "pos stall < pi/2", "pos beyond pi/2", "neg stall > -pi/2", "neg beyond -pi/2")


class _K:
    """The surface's constants in one dtype."""

    def __init__(self, S, dtype):
        f = dtype
        self.dtype = f
        for name in ("Cl_alpha_3D", "aero_tau", "eta", "flap_to_chord", "alpha_0_base", "alpha_stall_P_base", "alpha_stall_N_base", "Cd_0",
                     "deflection_limit", "aspect", "half_rho", "area", "chord"):
            setattr(self, name, f(getattr(S, name)))
        self.r, self.lift, self.drag, self.torque = (np.array(list(v), dtype=f) for v in (S.r, S.lift_unit, S.drag_unit, S.torque_unit))
        self.pi = f(np.pi)


def _arr(x, dtype):
    return np.asarray(x, dtype=dtype)


def _deflection(K, act):
    return (act * K.deflection_limit) * (K.pi / K.dtype(180.0))  # np.deg2rad, :386


def stall_angles(S, act, dtype=np.float64):
    """(alpha_0, alpha_stall_P, alpha_stall_N) of the deflected surface, lifting_surfaces.py:386-394."""
    K = S if isinstance(S, _K) else _K(S, dtype)
    act = _arr(act, K.dtype)
    defl = _deflection(K, act)
    dCl = K.Cl_alpha_3D * K.aero_tau * K.eta * defl
    dCl_max = K.flap_to_chord * dCl
    Cl_max_P = K.Cl_alpha_3D * (K.alpha_stall_P_base - K.alpha_0_base) + dCl_max
    Cl_max_N = K.Cl_alpha_3D * (K.alpha_stall_N_base - K.alpha_0_base) + dCl_max
    a0 = K.alpha_0_base - (dCl / K.Cl_alpha_3D)
    return a0, a0 + (Cl_max_P / K.Cl_alpha_3D), a0 + (Cl_max_N / K.Cl_alpha_3D)


def regime(S, alpha, act):
    """LINEAR .. NEG_BEYOND per point, from the float64 stall angles."""
    alpha, act = np.broadcast_arrays(_arr(alpha, np.float64), _arr(act, np.float64))
    _, aP, aN = stall_angles(S, act)
    lin = (aN < alpha) & (alpha < aP)
    pos = alpha > 0.0
    return np.where(lin, LINEAR, np.where(pos, np.where(alpha < np.pi / 2, POS_STALL, POS_BEYOND), np.where(alpha > -np.pi / 2, NEG_STALL, NEG_BEYOND)))


def induced_angle(S, alpha, act, dtype=np.float64):
    """alpha_i, :397-399 linear, :409-425 the two-point np.interp between the stall angle and +-pi/2 (clamped at its ends)."""
    K = S if isinstance(S, _K) else _K(S, dtype)
    f = K.dtype
    alpha, act = np.broadcast_arrays(_arr(alpha, f), _arr(act, f))
    alpha, act = alpha.ravel(), act.ravel()
    a0, aP, aN = stall_angles(K, act)
    lin = (aN < alpha) & (alpha < aP)
    ai = (K.Cl_alpha_3D * (alpha - a0)) / (K.pi * K.aspect)
    half_pi = K.pi / f(2.0)
    # np.interp takes one breakpoint pair per call: one call per distinct actuation and side
    for u in np.unique(act):
        m = (act == u) & ~lin
        if not m.any():
            continue
        u0, uP, uN = stall_angles(K, u)
        mp, mn = m & (alpha > 0), m & ~(alpha > 0)
        at_P = (K.Cl_alpha_3D * (uP - u0)) / (K.pi * K.aspect)
        at_N = (K.Cl_alpha_3D * (uN - u0)) / (K.pi * K.aspect)
        ai[mp] = np.interp(alpha[mp], [uP, half_pi], [at_P, 0.0]).astype(f)
        ai[mn] = np.interp(alpha[mn], [-half_pi, uN], [0.0, at_N]).astype(f)
    return ai, lin


def coefficients(S, alpha, act, dtype=np.float64):
    """(Cl, Cd, CM) at angle of attack alpha [rad] and actuation act in [-1, 1], lifting_surfaces.py:349-448."""
    K = S if isinstance(S, _K) else _K(S, dtype)
    f = K.dtype
    shape = np.broadcast(np.asarray(alpha), np.asarray(act)).shape
    alpha, act = np.broadcast_arrays(_arr(alpha, f), _arr(act, f))
    alpha, act = alpha.ravel(), act.ravel()
    a0, _, _ = stall_angles(K, act)
    ai, lin = induced_angle(K, alpha, act)
    ae = alpha - a0 - ai
    se, ce = np.sin(ae), np.cos(ae)
    # linear, :397-406
    Cl_l = K.Cl_alpha_3D * (alpha - a0)
    CT_l = K.Cd_0 * ce
    CN_l = (Cl_l + (CT_l * se)) / ce
    Cd_l = (CN_l * se) + (CT_l * ce)
    CM_l = -CN_l * (f(0.25) - (f(0.175) * (f(1.0) - ((f(2.0) * ae) / K.pi))))
    # post-stall, :427-448
    defl = _deflection(K, act)
    Cd_90 = (f(-4.26e-2) * (defl * defl)) + (f(2.1e-1) * defl) + f(1.98)
    CN_s = Cd_90 * se * (f(1.0) / (f(0.56) + f(0.44) * np.abs(se)) - f(0.41) * (f(1.0) - np.exp(f(-17.0) / K.aspect)))
    CT_s = f(0.5) * K.Cd_0 * ce
    Cl_s = (CN_s * ce) - (CT_s * se)
    Cd_s = (CN_s * se) + (CT_s * ce)
    CM_s = -CN_s * (f(0.25) - (f(0.175) * (f(1.0) - ((f(2.0) * np.abs(ae)) / K.pi))))
    out = (np.where(lin, Cl_l, Cl_s), np.where(lin, Cd_l, Cd_s), np.where(lin, CM_l, CM_s))
    assert all(o.dtype == f for o in out)
    return tuple(o.reshape(shape) for o in out)


def local_velocity(S, vb, wb, dtype=np.float64, r=None):
    """The surface link's velocity in the body frame: vb + wb x r (lifting_surfaces.py:73-110 with the link rigidly on the base).
    r: the link position to use instead of S.r (the float32 value a device holds, when the arithmetic alone is under test)."""
    K = S if isinstance(S, _K) else _K(S, dtype)
    return _arr(vb, K.dtype) + np.cross(_arr(wb, K.dtype), K.r if r is None else _arr(r, K.dtype))


def angle_of_attack(S, vloc, dtype=np.float64):
    K = S if isinstance(S, _K) else _K(S, dtype)
    vloc = _arr(vloc, K.dtype)
    return np.arctan2(-(vloc @ K.lift), vloc @ K.drag)  # :342-345


def force_torque(S, vloc, act, dtype=np.float64):
    """(F, T) in the link frame from the local velocity (..., 3), lifting_surfaces.py:326-347 and :450-498."""
    K = S if isinstance(S, _K) else _K(S, dtype)
    vloc = _arr(vloc, K.dtype)
    speed = np.sqrt((vloc * vloc).sum(-1))
    alpha = angle_of_attack(K, vloc)
    Cl, Cd, CM = coefficients(K, alpha, act)
    Q_area = (K.half_rho * (speed * speed)) * K.area
    lift, drag = Cl * Q_area, Cd * Q_area
    fn = (lift * np.cos(alpha)) + (drag * np.sin(alpha))
    fp = (lift * np.sin(alpha)) - (drag * np.cos(alpha))
    F = K.lift * fn[..., None] + K.drag * fp[..., None]
    T = (Q_area * CM * K.chord)[..., None] * K.torque
    return F, T


def wrench_about_base(S, vb, wb, act, dtype=np.float64):
    """(F, tau): the surface's force and its torque about the base origin, T + r x F, in the body frame."""
    K = S if isinstance(S, _K) else _K(S, dtype)
    F, T = force_torque(K, local_velocity(K, vb, wb), act)
    return F, T + np.cross(K.r, F)


# ------------------------------------------------------------------------------------------------ the sweep and its bound
# Shared by tests/test_cpu_aero_ref.py (the restatement against the oracle on these points; census and boundary share from the
# reference alone) and tests/test_gpu_aero.py (the device's forms on the same points).
ACTUATIONS = (-1.0, -0.5, -0.35, 0.0, 0.3, 0.5, 1.0)
SPEEDS = (1.0, 10.0, 40.0)
OFFSETS = (0.0, 1e-4, -1e-4, 1e-3, -1e-3)
N_GRID = 2049
# The device's angle of attack against the exact one: the polynomial atan2's stated 1.2e-7, half a float32 ulp at pi (1.2e-7), the
# float32 rounding of the stall angles it is compared with (3e-8 at 0.26 rad and at the deflection shift), doubled -> 4e-7 rad.
DELTA_ALPHA = 4e-7
JUMP = 1e-4  # a sensitivity above this: the point is within DELTA_ALPHA of a discontinuity of the coefficient
CENSUS = ("linear", "positive stall below pi/2", "positive beyond pi/2", "negative stall above -pi/2", "negative beyond -pi/2", "reversed flow")


def wrap(alpha):
    """Into (-pi, pi]."""
    return -((-np.asarray(alpha, np.float64) + np.pi) % (2.0 * np.pi) - np.pi)


def sweep(S):
    """(alpha, act, V, offset) of one surface: for every actuation the even grid on (-pi, pi] and, around each of aN, aP, +-pi/2, 0, +-pi,
    the offsets 0, +-1e-4, +-1e-3 rad; every speed. offset is NaN on the grid."""
    grid = -np.pi + 2.0 * np.pi * np.arange(1, N_GRID + 1) / N_GRID
    grid[-1] = np.pi
    al, ac, of = [], [], []
    for act in ACTUATIONS:
        _, aP, aN = stall_angles(S, act)
        centres = np.array([aN, aP, np.pi / 2, -np.pi / 2, 0.0, np.pi, -np.pi])
        extra = (centres[:, None] + np.array(OFFSETS)[None, :]).ravel()
        extra = np.where(np.abs(extra) > np.pi, wrap(extra), extra)  # (-pi itself stays: the lower side of the branch cut)
        a = np.concatenate([grid, extra])
        al.append(a); ac.append(np.full(a.shape, act)); of.append(np.concatenate([np.full(grid.shape, np.nan), np.tile(OFFSETS, len(centres))]))
    al, ac, of = np.concatenate(al), np.concatenate(ac), np.concatenate(of)
    n = len(al)
    return np.tile(al, len(SPEEDS)), np.tile(ac, len(SPEEDS)), np.repeat(SPEEDS, n), np.tile(of, len(SPEEDS))


def velocity(S, alpha, V, out_of_plane=0.0):
    """float32 local velocity with fa = V cos(alpha), la = -V sin(alpha) along the surface's forward and lift units (both axis-aligned
    in every model here, so the float32 components ARE fa and la) and out_of_plane along its torque unit."""
    K = _K(S, np.float64)
    fa, la = V * np.cos(alpha), -V * np.sin(alpha)
    v = fa[:, None] * K.drag + la[:, None] * K.lift + np.broadcast_to(out_of_plane, fa.shape)[:, None] * K.torque
    return v.astype(np.float32)


def census(S, vloc, act):
    """Points per CENSUS class, classified by the float64 reference at the velocities the device is given."""
    K = _K(S, np.float64)
    v = np.asarray(vloc, np.float64)
    reg = regime(S, angle_of_attack(S, v), act)
    counts = [int((reg == k).sum()) for k in range(5)]
    return counts + [int(((v @ K.drag) < 0).sum())]


def sensitivity(S, alpha, act, delta=DELTA_ALPHA):
    """max |C(alpha +- delta) - C(alpha)| per coefficient, (3, N), and the coefficients at alpha - delta, alpha, alpha + delta."""
    c0 = np.array(coefficients(S, alpha, act))
    cm = np.array(coefficients(S, wrap(alpha - delta), act))
    cp = np.array(coefficients(S, wrap(alpha + delta), act))
    return np.maximum(np.abs(cm - c0), np.abs(cp - c0)), (cm, c0, cp)


def recover(S, vloc, F, T):
    """(Cl, Cd, CM) in float64 from a force and a link-frame torque: L = fn ca + fp sa, D = fn sa - fp ca, CM = tm / (QA chord), with
    (ca, sa) and QA from the velocity the evaluation was given."""
    K = _K(S, np.float64)
    v, F, T = (np.asarray(x, np.float64) for x in (vloc, F, T))
    la, fa = v @ K.lift, v @ K.drag
    h = np.hypot(la, fa)
    ca, sa = fa / h, -la / h
    QA = K.half_rho * (v * v).sum(-1) * K.area
    fn, fp, tm = F @ K.lift, F @ K.drag, T @ K.torque
    return np.array([(fn * ca + fp * sa) / QA, (fn * sa - fp * ca) / QA, tm / (QA * K.chord)])


def e32(S, vloc, act, reg, smooth):
    """E32[output, regime]: the float32 restatement against the float64 one, both through recover(), over the smooth points, and
    max |ref| alongside."""
    c64 = np.array(coefficients(S, angle_of_attack(S, np.asarray(vloc, np.float64)), act))
    F32, T32 = force_torque(S, vloc, act, dtype=np.float32)
    assert F32.dtype == np.float32 and T32.dtype == np.float32
    c32 = recover(S, vloc, F32, T32)
    E, M = np.zeros((3, 5)), np.zeros((3, 5))
    for k in range(5):
        m = (reg == k) & smooth
        if m.any():
            E[:, k] = np.abs(c32 - c64)[:, m].max(1)
            M[:, k] = np.abs(c64)[:, m].max(1)
    return E, M


def coefficient_bound(sens, E, M, reg, margin=8.0):
    """sens + margin * max(E32, 2^-24 max|ref|) per output and point (the convention of test_gpu_mlp.bound_ratio)."""
    return sens + margin * np.maximum(E, 2.0 ** -24 * M)[:, reg]

"""TEST INFRASTRUCTURE: the attitude helpers of pyflyt_amd/csrc/uav_device.hpp as plain vectorised numpy -- np.arctan2, np.arcsin,
np.sin, np.cos, no kernel tricks -- in float64, or with every input and operation in float32 (`dtype=np.float32`: what rounding the
formulas in single precision costs, the E32 of tests/test_gpu_attitude.py's bound).

The point generators that the CPU and the GPU tests share are here too. Every point is rounded to float32, and the reference is
evaluated at the rounded value. tests/test_cpu_attitude_ref.py pins the float64 path to the line-by-line C oracle and prints the
E32 tables; tests/test_gpu_attitude.py and tests/test_gpu_attitude_outputs.py hold the device against it.

Quaternions are (x, y, z, w), arrays of shape (N, 4); Euler angles (roll, pitch, yaw), shape (N, 3)."""
import numpy as np

f32, f64 = np.float32, np.float64
EPS = 2.0 ** -24
THRESHOLD = 0.99999          # pybullet's gimbal-lock branch: |sarg| >= 0.99999
JUMP = 4.0 * EPS             # a point whose float64 sarg is within this of the threshold is "on a jump"
COS_EDGES = (0.0045, 0.01, 0.03, 0.1, 0.3)
# bins of the attitude functions. 0: below the census (the threshold family evaluated on the smooth side), 1-5: the census bins of
# cos(pitch), 6: the gimbal branch
BIN_NAMES = ("[thr, 0.0045)", "[0.0045, 0.01)", "[0.01, 0.03)", "[0.03, 0.1)", "[0.1, 0.3)", "[0.3, 1]", "gimbal")
N_BINS = 7
GIMBAL_BIN = 6
ATAN_BIN_NAMES = ("[0, pi/4)", "[pi/4, pi/2)", "[pi/2, 3pi/4)", "[3pi/4, pi]")


def wrap(a):
    """a folded to [-pi, pi): the difference of two angles."""
    return (np.asarray(a, f64) + np.pi) % (2.0 * np.pi) - np.pi


# ------------------------------------------------------------------------------------------------ the reference
def sarg_of(q, dtype=f64):
    """sin(pitch) = -2 (x z - w y) / |q|^2, as getEulerFromQuaternion takes it."""
    q = np.asarray(q, dtype)
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return dtype(-2.0) * (x * z - w * y) / (x * x + y * y + z * z + w * w)


def euler_smooth(q, dtype=f64):
    """The branch away from the poles, at every point."""
    q = np.asarray(q, dtype)
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    sx, sy, sz, sw = x * x, y * y, z * z, w * w
    s = np.clip(sarg_of(q, dtype), dtype(-1.0), dtype(1.0))
    two = dtype(2.0)
    return np.stack([np.arctan2(two * (y * z + w * x), sw - sx - sy + sz), np.arcsin(s), np.arctan2(two * (x * y + w * z), sw + sx - sy - sz)], 1)


def euler_gimbal(q, dtype=f64):
    """The gimbal-lock branch, at every point: roll 0, pitch +-pi/2 by the sign of sarg, yaw 2 atan2(+-x, -+y)."""
    q = np.asarray(q, dtype)
    x, y = q[:, 0], q[:, 1]
    up = sarg_of(q, dtype) > 0
    half_pi = dtype(0.5) * dtype(np.pi)
    yaw = dtype(2.0) * np.where(up, np.arctan2(-x, y), np.arctan2(x, -y))
    return np.stack([np.zeros_like(x), np.where(up, half_pi, -half_pi), yaw], 1)


def in_gimbal(q, dtype=f64):
    return np.abs(sarg_of(q, dtype)) >= dtype(THRESHOLD)


def euler_from_quat(q, dtype=f64):
    """pybullet getEulerFromQuaternion (ZYX), both gimbal branches."""
    return np.where(in_gimbal(q, dtype)[:, None], euler_gimbal(q, dtype), euler_smooth(q, dtype))


def quat_from_euler(e, dtype=f64):
    """pybullet getQuaternionFromEuler, normalised."""
    e = np.asarray(e, dtype)
    h = dtype(0.5)
    sr, cr, sp, cp, sy, cy = np.sin(h * e[:, 0]), np.cos(h * e[:, 0]), np.sin(h * e[:, 1]), np.cos(h * e[:, 1]), np.sin(h * e[:, 2]), np.cos(h * e[:, 2])
    q = np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy], 1)
    return q / np.sqrt((q * q).sum(1, dtype=dtype))[:, None]


def canon(q, dtype=f64, branch=None):
    """quat_from_euler(euler_from_quat(q)); branch: "smooth" / "gimbal" forces that branch at every point."""
    e = euler_from_quat(q, dtype) if branch is None else (euler_smooth if branch == "smooth" else euler_gimbal)(q, dtype)
    return quat_from_euler(e, dtype)


def matrix_from_quat(q, dtype=f64):
    """btMatrix3x3::setRotation: body -> world, with the 2 / |q|^2 scale. (N, 3, 3)."""
    q = np.asarray(q, dtype)
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    s = dtype(2.0) / (x * x + y * y + z * z + w * w)
    xs, ys, zs = x * s, y * s, z * s
    wx, wy, wz, xx, xy, xz, yy, yz, zz = w * xs, w * ys, w * zs, x * xs, x * ys, x * zs, y * ys, y * zs, z * zs
    one = dtype(1.0)
    return np.stack([one - (yy + zz), xy - wz, xz + wy, xy + wz, one - (xx + zz), yz - wx, xz - wy, yz + wx, one - (xx + yy)], 1).reshape(-1, 3, 3)


def qmul(a, b):
    """Hamilton product a (x) b, (x, y, z, w)."""
    av, aw, bv, bw = a[:, :3], a[:, 3:], b[:, :3], b[:, 3:]
    return np.concatenate([aw * bv + bw * av + np.cross(av, bv), aw * bw - (av * bv).sum(1, keepdims=True)], 1)


def exp_map_step(q, w, half_dt, dtype=f64):
    """exp(w dt / 2) (x) q, normalised: the exact step btMultiBody::stepPositionsMultiDof takes."""
    q, w = np.asarray(q, dtype), np.asarray(w, dtype)
    wn = np.sqrt((w * w).sum(1, dtype=dtype))
    th = wn * dtype(half_dt)
    with np.errstate(invalid="ignore", divide="ignore"):
        axis = np.where(wn[:, None] > 0, w / wn[:, None], dtype(0.0))
    dq = np.concatenate([axis * np.sin(th)[:, None], np.cos(th)[:, None]], 1).astype(dtype)
    n = qmul(dq, q)
    return n / np.sqrt((n * n).sum(1, dtype=dtype))[:, None]


def half_angle(c, s, dtype=f64):
    """(cos(t/2), sin(t/2)) of the angle t = atan2(s, c) in (-pi, pi]."""
    t = np.arctan2(np.asarray(s, dtype), np.asarray(c, dtype))
    return np.cos(dtype(0.5) * t), np.sin(dtype(0.5) * t)


# ------------------------------------------------------------------------------------------------ bins and jumps
def attitude_bins(q):
    """(bin, on_jump) per point from the float64 sarg at the float32 input."""
    s = np.abs(sarg_of(q))
    cosp = np.sqrt(np.maximum(1.0 - s * s, 0.0))
    b = np.searchsorted(np.array(COS_EDGES), cosp, side="right")  # 0 below the first edge .. 5 from 0.3 up
    b = np.where(s >= THRESHOLD, GIMBAL_BIN, b)
    return b, np.abs(s - THRESHOLD) <= JUMP


def atan_bins(r):
    return np.minimum((np.abs(r) / (np.pi / 4)).astype(int), 3)


def per_bin_max(err, bins, n_bins):
    """max of err (N,) or (N, K) per bin -> (n_bins,) or (n_bins, K); 0 for an empty bin."""
    err = np.asarray(err, f64)
    out = np.zeros((n_bins,) + err.shape[1:])
    for b in range(n_bins):
        m = bins == b
        if m.any():
            out[b] = err[m].max(0)
    return out


def bound(T, M, E32, maxref):
    """T + M max(E32, 2^-24 max|ref|), per bin (and output)."""
    return T + M * np.maximum(E32, EPS * maxref)


# ------------------------------------------------------------------------------------------------ the primitives' float32 chains
# The device's own operation chain in numpy float32: an fma is the float64 product and sum rounded once (exact to double rounding), a
# division stands where the device multiplies by v_rcp_f32, np.sqrt where it takes v_sqrt_f32 / v_rsq_f32.
ATAN_COEF = (0.0029035410843789577, -0.016282962635159492, 0.04303929582238197, -0.07533670216798782, 0.10654674470424652,
             -0.14207133650779724, 0.19993053376674652, -0.3333309292793274, 1.0)  # fast_atan2, highest degree first
SIN_COEF = (-2.5052108e-8, 2.7557319e-6, -1.9841270e-4, 8.3333333e-3, -1.6666667e-1, 1.0)
COS_COEF = (2.0876757e-9, -2.7557319e-7, 2.4801587e-5, -1.3888889e-3, 4.1666667e-2, -0.5, 1.0)
SINC_COEF = (2.7557319e-6, -1.9841270e-4, 8.3333333e-3, -1.6666667e-1, 1.0)           # quat_integrate: sin(t)/t in t^2
COSQ_COEF = (-2.7557319e-7, 2.4801587e-5, -1.3888889e-3, 4.1666667e-2, -0.5, 1.0)     # quat_integrate: cos(t) in t^2
PI32 = f32(np.pi)


def fma32(a, b, c):
    return (np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64) + np.asarray(c, f32).astype(f64)).astype(f32)


def horner32(s, coef):
    p = np.full_like(s, f32(coef[0]))
    for c in coef[1:]:
        p = fma32(s, p, f32(c))
    return p


def horner64(s, coef):
    """The float32 coefficients, evaluated in float64: the polynomial itself."""
    p = np.full_like(s, f64(f32(coef[0])))
    for c in coef[1:]:
        p = p * s + f64(f32(c))
    return p


def fast_atan2_f32(y, x):
    y, x = np.asarray(y, f32), np.asarray(x, f32)
    ax, ay = np.abs(x), np.abs(y)
    mx, mn = np.maximum(ax, ay), np.minimum(ax, ay)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(mx == 0, f32(0.0), mn / mx).astype(f32)
    r = horner32(t * t, ATAN_COEF) * t
    r = np.where(ay > ax, f32(0.5) * PI32 - r, r)
    r = np.where(x < 0, PI32 - r, r)
    return np.copysign(r, y).astype(f32)


def fast_asin_f32(x):
    x = np.asarray(x, f32)
    return fast_atan2_f32(x, np.sqrt(np.maximum((f32(1.0) - x) * (f32(1.0) + x), f32(0.0))))


def atan_truncation(n=200001):
    """max |p(t^2) t - atan t| on [0, 1], float32 coefficients, float64 evaluation."""
    t = np.linspace(0.0, 1.0, n)
    return float(np.abs(horner64(t * t, ATAN_COEF) * t - np.arctan(t)).max())


def sincos_small_f32(x):
    x = np.asarray(x, f32)
    t = x * x
    return (x * horner32(t, SIN_COEF)).astype(f32), horner32(t, COS_COEF)


def sincos_truncation(lim, n=200001):
    """max over [-lim, lim] of |polynomial - function| for sincos_small's pair."""
    x = np.linspace(-lim, lim, n)
    t = x * x
    return float(np.abs(x * horner64(t, SIN_COEF) - np.sin(x)).max()), float(np.abs(horner64(t, COS_COEF) - np.cos(x)).max())


def sincos_turns_f32(u):
    u = np.asarray(u, f32)
    k = np.rint(f32(4.0) * u).astype(f32)
    r = (f32(2.0) * PI32) * fma32(k, f32(-0.25), u)
    s, c = sincos_small_f32(r)
    q = k.astype(int) & 3
    odd = (q & 1) != 0
    a, b = np.where(odd, c, s), np.where(odd, s, c)
    return np.where((q & 2) != 0, -a, a).astype(f32), np.where((q == 1) | (q == 2), -b, b).astype(f32)


def sincos_angle_f32(a):
    """dogfight.hpp's wrapper: an angle in [-pi, pi] -> turns in [0, 1]."""
    a = np.asarray(a, f32)
    u = a * (f32(0.5) / PI32)
    return sincos_turns_f32(u - np.floor(u))


def half_angle_f32(c, s):
    c, s = np.asarray(c, f32), np.asarray(s, f32)
    a = np.sqrt(f32(0.5) * (f32(1.0) + np.abs(c)))
    b = f32(0.5) * s / a
    pos = c >= 0
    return np.where(pos, a, np.abs(b)).astype(f32), np.where(pos, b, np.copysign(a, s)).astype(f32)


def quat_integrate_f32(q, w, half_dt):
    q, w, h = np.asarray(q, f32), np.asarray(w, f32), f32(half_dt)
    dot = fma32(w[:, 0], w[:, 0], fma32(w[:, 1], w[:, 1], w[:, 2] * w[:, 2]))
    t2 = dot * (h * h)
    k = horner32(t2, SINC_COEF) * h
    c = horner32(t2, COSQ_COEF)
    ax, ay, az = w[:, 0] * k, w[:, 1] * k, w[:, 2] * k
    x, y, z, s = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    n = np.stack([fma32(c, x, fma32(ax, s, fma32(ay, z, -(az * y)))), fma32(c, y, fma32(ay, s, fma32(az, x, -(ax * z)))),
                  fma32(c, z, fma32(az, s, fma32(ax, y, -(ay * x)))), fma32(c, s, fma32(-ax, x, fma32(-ay, y, -(az * z))))], 1)
    d = fma32(n[:, 0], n[:, 0], fma32(n[:, 1], n[:, 1], fma32(n[:, 2], n[:, 2], n[:, 3] * n[:, 3])))
    return (n * (f32(1.0) / np.sqrt(d))[:, None]).astype(f32)


def integrate_truncation(n=20001):
    """max over theta in [0, pi/8] of the two polynomials' own errors (sin t / t, cos t)."""
    t = np.linspace(1e-9, np.pi / 8, n)
    return float(np.abs(horner64(t * t, SINC_COEF) - np.sin(t) / t).max()), float(np.abs(horner64(t * t, COSQ_COEF) - np.cos(t)).max())


# ------------------------------------------------------------------------------------------------ the points
def _quat_of(roll, pitch, yaw):
    return quat_from_euler(np.stack([roll, pitch, yaw], 1)).astype(f32)


def _quat_at_sarg(s, roll, yaw):
    """A float32 unit quaternion whose sin(pitch) is s to float32 rounding of the components."""
    return _quat_of(roll, np.arcsin(np.clip(s, -1.0, 1.0)), yaw)


class Attitudes:
    """The attitude points, by family (slices into .q, float32 unit quaternions), and the non-unit scalings of the Haar set."""

    LADDER_K = tuple(1.0 + 0.25 * i for i in range(16))  # 1.0, 1.25 .. 4.75

    def __init__(self, seed=20):
        rng = np.random.default_rng(seed)
        fam = {}
        h = rng.normal(size=(4096, 4))
        fam["haar"] = (h / np.linalg.norm(h, axis=1, keepdims=True)).astype(f32)
        lad = []
        for k in self.LADDER_K:
            for sign in (1.0, -1.0):
                lad.append(_quat_at_sarg(np.full(128, sign * (1.0 - 10.0 ** -k)), rng.uniform(-np.pi, np.pi, 128), rng.uniform(-np.pi, np.pi, 128)))
        fam["ladder"] = np.concatenate(lad)
        gim, thr = [], []
        for sign in (1.0, -1.0):
            # well inside the gimbal branch: pitch exactly +-pi/2, and |sarg| between 0.999995 and 1
            gim.append(_quat_of(rng.uniform(-np.pi, np.pi, 32), np.full(32, sign * np.pi / 2), rng.uniform(-np.pi, np.pi, 32)))
            gim.append(_quat_at_sarg(sign * rng.uniform(0.999995, 1.0, 32), rng.uniform(-np.pi, np.pi, 32), rng.uniform(-np.pi, np.pi, 32)))
            j = np.resize(np.arange(-8, 9), 64)
            thr.append(_quat_at_sarg(sign * THRESHOLD * (1.0 + j * EPS), rng.uniform(-np.pi, np.pi, 64), rng.uniform(-np.pi, np.pi, 64)))
        fam["gimbal"], fam["threshold"] = np.concatenate(gim), np.concatenate(thr)
        # yaw and roll at 0, +-pi/2, +-pi: the angle, its float32 neighbours, +-1e-6; eight random partners each
        special = []
        for a in (0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi):
            a32 = f32(a)
            special += [f64(a32), f64(np.nextafter(a32, f32(np.inf))), f64(np.nextafter(a32, f32(-np.inf))), a + 1e-6, a - 1e-6]
        special = np.repeat(np.array(special), 8)
        m = len(special)
        fam["yaw"] = _quat_of(rng.uniform(-np.pi, np.pi, m), rng.uniform(-1.2, 1.2, m), special)
        fam["roll"] = _quat_of(special, rng.uniform(-1.2, 1.2, m), rng.uniform(-np.pi, np.pi, m))
        fam["identity"] = np.array([[0, 0, 0, 1], [0, 0, 0, -1]], f32)
        fam["half_turns"] = np.array([[1, 0, 0, 0], [-1, 0, 0, 0], [0, 1, 0, 0], [0, -1, 0, 0], [0, 0, 1, 0], [0, 0, -1, 0]], f32)
        self.family, parts, at = {}, [], 0
        for name, q in fam.items():
            self.family[name] = slice(at, at + len(q))
            parts.append(q)
            at += len(q)
        self.q = np.concatenate(parts)
        self.n = at
        # non-unit inputs, for the functions that keep |q|^2 only
        self.scaled = {0.5: (fam["haar"].astype(f64) * 0.5).astype(f32), 1.37: (fam["haar"].astype(f64) * 1.37).astype(f32)}

    def all_points(self):
        """Unit and scaled, one array: what euler_from_quat, euler_from_quat_fast, canon_quat and rot_from_quat are run on."""
        return np.concatenate([self.q, self.scaled[0.5], self.scaled[1.37]])


def atan2_points(seed=21):
    """(y, x) float32: 2^18 random points, then the deliberate ones (axes, diagonals, both sides of every octant boundary, signed zeros)."""
    rng = np.random.default_rng(seed)
    n = 1 << 18
    mag = 10.0 ** rng.uniform(-18.0, 18.0, n)
    ang = rng.uniform(-np.pi, np.pi, n)
    y, x = (mag * np.sin(ang)).astype(f32), (mag * np.cos(ang)).astype(f32)
    ey, ex = [], []
    tiny = np.finfo(f32).tiny  # the smallest normal: one step off an axis without a denormal
    for m in (1e-18, 1e-6, 0.3, 1.0, 1.5, 777.0, 1e18):
        m = f32(m)
        up, dn = np.nextafter(m, f32(np.inf)), np.nextafter(m, f32(0.0))
        for sy in (1.0, -1.0):
            for sx in (1.0, -1.0):
                for a, b in ((m, m), (up, m), (dn, m), (m, up), (m, dn)):   # the diagonal, one ulp either side
                    ey.append(sy * a); ex.append(sx * b)
        for s in (1.0, -1.0):
            for a, b in ((0.0, s * m), (-0.0, s * m), (s * m, 0.0), (s * m, -0.0)):  # the axes, signed zeros
                ey.append(a); ex.append(b)
            for t in (tiny, -tiny):                                                   # one normal step off each axis
                ey.append(t * max(float(m), 1.0)); ex.append(s * max(float(m), 1.0))
                ey.append(s * max(float(m), 1.0)); ex.append(t * max(float(m), 1.0))
    ey += [0.0, -0.0]
    ex += [0.0, 0.0]
    y, x = np.concatenate([y, np.array(ey, f32)]), np.concatenate([x, np.array(ex, f32)])
    ok = lambda v: (v == 0) | (np.abs(v) >= tiny)  # noqa: E731  (no denormals: nothing produces them)
    keep = ok(y) & ok(x) & np.isfinite(y) & np.isfinite(x)
    return y[keep], x[keep]


def asin_points():
    """[-1, 1], dense near +-1."""
    lin = np.linspace(-1.0, 1.0, 1 << 16)
    near = 1.0 - 10.0 ** np.linspace(-8.0, -0.5, 1 << 14)
    one = f32(1.0)
    steps = [one]
    for _ in range(64):
        steps.append(np.nextafter(steps[-1], f32(0.0)))
    steps = np.array(steps, f64)
    return np.unique(np.concatenate([lin, near, -near, steps, -steps, [0.0]]).astype(f32))


def small_points():
    """sincos_small's domain [-1, 1]."""
    return np.unique(np.concatenate([np.linspace(-1.0, 1.0, (1 << 16) + 1), [0.8, -0.8, np.pi / 4, -np.pi / 4]]).astype(f32))


def turn_points():
    """u on a 2^16 grid of [0, 1], every k/8 exactly and its two float32 neighbours (inside [0, 1])."""
    g = np.linspace(0.0, 1.0, (1 << 16) + 1).astype(f32)
    e = []
    for k in range(9):
        u = f32(k / 8.0)
        e += [u, np.nextafter(u, f32(2.0)), np.nextafter(u, f32(-1.0))]
    e = np.array(e, f32)
    return np.concatenate([g, e[(e >= 0) & (e <= 1)]])


def angle_points():
    """dogfight.hpp's wrapper: [-pi, pi], including +-pi (float32), +-0 and -1e-9."""
    g = np.linspace(-np.pi, np.pi, (1 << 16) + 1).astype(f32)
    g = np.clip(g, -PI32, PI32)
    return np.concatenate([g, np.array([PI32, -PI32, 0.0, -0.0, -1e-9, 1e-9, np.pi / 2, -np.pi / 2], f32)])


def half_angle_points(n=1 << 16):
    """(c, s) = (cos t, sin t), t dense in (-pi, pi], then c = +-1 with s = +-0, and c = 0."""
    t = np.linspace(-np.pi, np.pi, n + 1)[1:]
    c, s = np.cos(t).astype(f32), np.sin(t).astype(f32)
    ec = np.array([1, 1, -1, -1, 0, 0], f32)
    es = np.array([0.0, -0.0, 0.0, -0.0, 1, -1], f32)
    return np.concatenate([c, ec]), np.concatenate([s, es])


HALF_DT = 1.0 / 480.0
N_CORNERS, N_ZERO = 8, 16


def integration_points(att, seed=22):
    """(q, w) float32 on 1 024 of the Haar attitudes: the clamp corners (+-100, +-100, +-100), w = 0, then |w| log-uniform in
    1e-6 .. 100 sqrt(3) in a random direction."""
    rng = np.random.default_rng(seed)
    n = 1024
    q = att.q[att.family["haar"]][:n]
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    w = d * (10.0 ** rng.uniform(-6.0, np.log10(100.0 * np.sqrt(3.0)), n))[:, None]
    w[:N_CORNERS] = [[sx * 100.0, sy * 100.0, sz * 100.0] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    w[N_CORNERS:N_CORNERS + N_ZERO] = 0.0
    return q, w.astype(f32)


# ------------------------------------------------------------------------------------------------ the E32 tables
class AttitudeTables:
    """Per bin (and output): E32 and max|ref| of euler_from_quat, canon and matrix_from_quat on a set of points, from the reference
    in float32 against the reference in float64 at the same float32 inputs. Both branches are evaluated at every point (.smooth,
    .gimbal: Euler angles; .canon_smooth, .canon_gimbal); .euler / .canon take the float64 branch. In the zone around the threshold
    (64 x 2^-24 either side: the threshold family) either branch's formulas are sound, and a point on a jump may be held to either:
    there the smooth formulas' errors count towards bin 0 and the gimbal formulas' towards the gimbal bin, on both sides."""

    def __init__(self, q):
        q = np.asarray(q, f32)
        self.bins, self.jump = attitude_bins(q)
        gim = self.bins == GIMBAL_BIN
        zone = np.abs(np.abs(sarg_of(q)) - THRESHOLD) <= 64.0 * EPS
        as_smooth, as_gimbal = (~gim) | zone, gim | zone

        def table(smooth_err, gimbal_err):
            e = per_bin_max(np.where(as_smooth[:, None], smooth_err, 0.0), np.where(gim, 0, self.bins), N_BINS)
            e[GIMBAL_BIN] = np.where(as_gimbal[:, None], gimbal_err, 0.0).max(0)
            return e

        self.smooth, self.gimbal = euler_smooth(q), euler_gimbal(q)
        s32, g32 = euler_smooth(q, f32), euler_gimbal(q, f32)
        self.euler = np.where(gim[:, None], self.gimbal, self.smooth)
        self.e_euler = table(np.abs(wrap(s32.astype(f64) - self.smooth)), np.abs(wrap(g32.astype(f64) - self.gimbal)))
        self.m_euler = table(np.abs(self.smooth), np.abs(self.gimbal))
        self.canon_smooth, self.canon_gimbal = quat_from_euler(self.smooth), quat_from_euler(self.gimbal)
        self.canon = np.where(gim[:, None], self.canon_gimbal, self.canon_smooth)
        either = lambda a, b: np.minimum(np.abs(a - b), np.abs(a + b))  # noqa: E731  (either sign next to an atan2 of +-pi; the GPU test holds the sign)
        self.e_canon = table(either(quat_from_euler(s32, f32).astype(f64), self.canon_smooth), either(quat_from_euler(g32, f32).astype(f64), self.canon_gimbal))
        self.m_canon = table(np.abs(self.canon_smooth), np.abs(self.canon_gimbal))
        self.R = matrix_from_quat(q).reshape(-1, 9)
        self.e_R = per_bin_max(np.abs(matrix_from_quat(q, f32).reshape(-1, 9).astype(f64) - self.R), self.bins, N_BINS)
        self.m_R = per_bin_max(np.abs(self.R), self.bins, N_BINS)

    def widened_by(self, other):
        """This set's references and bins with E32 and max|ref| no smaller than `other`'s: a small set's own per-bin maxima understate
        what float32 costs in a bin it barely visits."""
        for k in ("e_euler", "m_euler", "e_canon", "m_canon", "e_R", "m_R"):
            setattr(self, k, np.maximum(getattr(self, k), getattr(other, k)))
        return self

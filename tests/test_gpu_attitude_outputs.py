"""The env kernels' own copies of the attitude code, through a dynamics-free identity: after one env step, the observation's attitude
and body-frame velocities must be the float64 functions (tests/attitude_ref.py) of the state that the same step stored.

tests/test_gpu_attitude.py holds the helpers of uav_device.hpp one by one. The kernels do not only call them: the two fast kernels
restate canon_quat and the Euler block inline in their write_obs_row, from the rotation matrix derive() holds instead of from q
(quadx_fast.hpp, fixedwing_fast.hpp), and the generic kernels cache the Euler angles behind an rpy_valid flag (env_generic.hpp,
rocket_landing.hpp). A matrix entry misnamed there, or a stale cached rpy, moves no trajectory test by more than its tolerance near
most attitudes -- here it fails at every lane.

Per configuration, with noise and auto-reset off: one lane per attitude point of attitude_ref.Attitudes (unit quaternions; identity
padding to a multiple of 64), env_reset(), the quaternion group overwritten with the points, random world-frame velocities (a few m/s;
angular: a few rad/s on the even lanes, a hundredth of that on the odd ones, so that half of the ladder towards the poles is still
near the poles after the step), one step with zero actions, the state read back. Then, with the bounds, bins and jump rules of
test_gpu_attitude.py, evaluated at the READ-BACK quaternion:

  attitude   the obs's Euler angles / canonical quaternion = euler_from_quat(q) / canon(q)
  vb, wb     = R(q)^T v, R(q)^T w: per component (bR + 3 x 2^-24) |v|_1 -- bR the rot_from_quat bound of the lane's bin on every
             entry (|R_ij| <= 1), three roundings of the fma chain whose partial sums stay under |v|_1
  p          = the stored position, bit for bit (the dogfight observes the body centre, 0.35 m behind the stored point: left out)
  Waypoints  target deltas = R(canon(q))^T (target - p), yaw errors = wrap(yaw target - yaw): see check_waypoints

The cascaded flight modes of the specialised QuadX kernel keep a float64 master of the rigid-body state in extra state groups; what
they observe is a function of that master, not of the float32 groups read back here: left out. The dogfight env observes Euler angles
only (the ABI refuses the quaternion representation for it)."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attitude_ref as R  # noqa: E402
import test_gpu_attitude as TA  # noqa: E402
from test_gpu_kat import base, set_w  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = R.EPS
f32, f64 = np.float32, np.float64


class Points:
    """The attitude set, padded; its designed tables (the E32 floor of every bin); the velocities."""

    def __init__(self):
        self.att = R.Attitudes()
        n = -(-self.att.n // 64) * 64
        self.q = np.tile(np.array([[0, 0, 0, 1]], f32), (n, 1))
        self.q[: self.att.n] = self.att.q
        self.n = n
        self.designed = R.AttitudeTables(self.att.all_points())
        rng = np.random.default_rng(31)
        self.v = rng.uniform(-3.0, 3.0, (n, 3)).astype(f32)
        self.w = rng.uniform(-3.0, 3.0, (n, 3)).astype(f32)
        self.w[1::2] *= f32(0.01)
        self.T_atan = R.atan_truncation()


@pytest.fixture(scope="module")
def pts():
    return Points()


class Held:
    """What test_gpu_attitude's checks take for a world: the points, their tables (widened by the designed set's), the polynomial's T."""

    def __init__(self, pts, q):
        self.q = np.ascontiguousarray(q, f32)
        self.tab = R.AttitudeTables(self.q).widened_by(pts.designed)
        self.T_atan = pts.T_atan


def one_step(pts, vehicle, task, representation, setup=None, ended=None, **kw):
    """ended: the state group that holds the lane's flags -- every lane is marked terminated before the step. With auto-reset off
    such a lane runs no Aviary step: its observation must still be that of the state it holds, which the generic kernels only get
    right by recomputing the Euler angles they otherwise cache from the last Aviary step (rpy_valid). The attitudes stay exactly
    the designed ones, the threshold family included."""
    from pyflyt_amd import _lib as L
    from pyflyt_amd import build_params
    from pyflyt_amd.engine import BatchEngine

    P = build_params(vehicle, task, noise="off", autoreset="off", angle_representation=representation, **kw)
    eng = BatchEngine(P, pts.n, device=DEV)
    if setup is not None:
        setup(eng)
    eng.env_reset()
    eng.state[1] = torch.tensor(pts.q, device=DEV)
    eng.state[2, :, :3] = torch.tensor(pts.v, device=DEV)
    set_w(eng, pts.w)
    if ended is not None:
        eng.state[ended].view(torch.int32)[:, 1] |= L.F_TERMINATED
    obs = eng.env_step(torch.zeros(pts.n, eng.action_dim, device=DEV))[0].double().cpu().numpy()
    p, q, v, w = base(eng)
    assert np.isfinite(obs).all() and np.isfinite(q).all()
    return eng, obs, p, q, v, w


def check_block(pts, name, obs, p, q, v, w, quat, position=True):
    """The attitude block [wb 3][attitude 3 or 4][vb 3][p 3] against the float64 functions of the read-back state. Returns the Held."""
    H = Held(pts, q)
    tab = H.tab
    na = 4 if quat else 3
    wb, att, vb, pp = obs[:, 0:3], obs[:, 3:3 + na], obs[:, 3 + na:6 + na], obs[:, 6 + na:9 + na]
    counts = [int((tab.bins == b).sum()) for b in range(R.N_BINS)]
    print(f"\n{name}: {len(q)} lanes; read-back attitudes per bin " + ", ".join(f"{n} {c}" for n, c in zip(R.BIN_NAMES, counts)) + f"; on a jump {int(tab.jump.sum())}")
    assert min(counts[1:6]) >= 100 and counts[R.GIMBAL_BIN] >= 32, counts  # (the step has not swept the poles empty)
    assert np.abs(np.linalg.norm(q, axis=1) - 1.0).max() <= 2e-7
    smooth = ~tab.jump
    if quat:
        Bc = TA.canon_bounds(H)
        err, b, near = TA.canon_err(H, att.astype(f32), "own")
        TA.held(name + " canon", "xyzw", err, Bc[b], b, R.BIN_NAMES, where=smooth)
        j = np.flatnonzero(tab.jump)
        es, bs, _ = TA.canon_err(H, att.astype(f32), "smooth")
        eg, bg, _ = TA.canon_err(H, att.astype(f32), "gimbal")
        ok = (es[j] <= Bc[bs[j]]).all(1) | (eg[j] <= Bc[bg[j]]).all(1)
        assert ok.all(), (name, "a lane on the jump matches neither side", q[j[~ok][0]], att[j[~ok][0]])
    else:
        TA.check_euler(H, name + " euler", att.astype(f32), True)
    # body-frame velocities
    BR = R.bound(0.0, TA.M_COMPOSITE, tab.e_R, tab.m_R)[tab.bins].max(1)
    R0 = tab.R.reshape(-1, 3, 3)
    for what, got, x in (("vb", vb, v), ("wb", wb, w)):
        bnd = (BR + 3 * EPS) * np.abs(x).sum(1)
        TA.held(name + " " + what, "xyz", np.abs(got - np.einsum("nji,nj->ni", R0, x)), np.repeat(bnd[:, None], 3, 1) + 1e-45, tab.bins, R.BIN_NAMES)
    if position:
        assert np.array_equal(pp.astype(f32).view(np.uint32), p.astype(f32).view(np.uint32)), name
    return H


def specialised(eng):
    return eng.lib.pf_ctx_is_specialised(eng._ctx) != 0


# ------------------------------------------------------------------------------------------------ QuadX-Hover, Fixedwing-Waypoints: both kernels
FLAGS_GROUP = {"quadx": 6, "fixedwing": 5, "rocket": 6}  # (QuadX::store, Fixedwing::store, Rocket::store: step count, flags, counter, targets left)


@pytest.mark.parametrize("lanes", ["flying", "ended"])
@pytest.mark.parametrize("representation", ["quaternion", "euler"])
@pytest.mark.parametrize("kernel", ["specialised", "generic"])
@pytest.mark.parametrize("vehicle,task", [("quadx", "hover"), ("fixedwing", "waypoints")])
def test_obs_is_the_float64_function_of_the_stored_state(pts, vehicle, task, kernel, representation, lanes, monkeypatch):
    if kernel == "generic":
        monkeypatch.setenv("PF_DISABLE_FAST", "1")
    eng, obs, p, q, v, w = one_step(pts, vehicle, task, representation, ended=FLAGS_GROUP[vehicle] if lanes == "ended" else None)
    assert specialised(eng) == (kernel == "specialised")
    if lanes == "ended":  # nothing moved
        assert np.array_equal(q.astype(f32), pts.q) and np.array_equal(v.astype(f32), pts.v) and np.array_equal(w.astype(f32), pts.w)
    check_block(pts, f"{vehicle}-{task} {kernel} {representation} {lanes}", obs, p, q, v, w, representation == "quaternion")
    TA.print_ratios(f"{vehicle}-{task}, {kernel} kernel, {representation}, lanes {lanes}")


# ------------------------------------------------------------------------------------------------ QuadX-Waypoints with yaw targets
def check_waypoints(pts, name, eng, H, obs, p, quat):
    """Target deltas R(canon(q))^T (t_i - p) and yaw errors wrap(yaw_i - yaw) of the live targets, lanes off the jump.
    The kernel rotates by rot_from_quat of ITS canonical quaternion qe: an error dq on qe's components moves an entry of R (two
    products 2 q_a q_b) by at most 2 x 2 (|q_a| + |q_b|) dq <= 4 sqrt(2) dq; with rot_from_quat's own bound bR on top the delta is
    off by (4 sqrt(2) dq + bR + 3 x 2^-24) |t - p|_1, and by 2^-24 |t - p|_1 for the rounding of t - p itself."""
    tab = H.tab
    st = eng.state
    tg = torch.cat([st[12], st[13], st[14]], dim=1).double().cpu().numpy().reshape(-1, 4, 3)
    yt = st[15].double().cpu().numpy()
    n_left = st[6, :, 3].view(torch.int32).cpu().numpy()
    full = n_left == 4  # (a target drawn within reach of the start is reached in this very step, and popped: those few lanes are left out)
    assert full.mean() >= 0.99, full.mean()
    na = 4 if quat else 3
    blk = obs[:, 9 + na + 8:].reshape(-1, 4, 4)
    ok = ~tab.jump & full
    Rc = R.matrix_from_quat(tab.canon)
    dq = TA.canon_bounds(H)[tab.bins].max(1)
    bR = R.bound(0.0, TA.M_COMPOSITE, tab.e_R, tab.m_R)[tab.bins].max(1)
    By = TA.euler_bounds(H, True)[tab.bins, 2]
    for i in range(4):
        d = tg[:, i] - p
        ref = np.einsum("nji,nj->ni", Rc, d)
        bnd = (4 * np.sqrt(2.0) * dq + bR + 4 * EPS) * np.abs(d).sum(1)
        TA.held(name + " target delta", "xyz", np.abs(blk[:, i, :3] - ref), np.repeat(bnd[:, None], 3, 1), tab.bins, R.BIN_NAMES, where=ok)
        # yaw_now() (quadx_fast.hpp) must agree with the Euler yaw: its error, and the roundings of the difference and of the wrap
        ey = np.abs(R.wrap(blk[:, i, 3] - (yt[:, i] - tab.euler[:, 2])))
        TA.held(name + " yaw error", ("yaw",), ey, By + 2 * EPS * (np.abs(yt[:, i]) + 2 * np.pi), tab.bins, R.BIN_NAMES, where=ok)
        assert (np.abs(blk[:, i, 3]) <= np.pi + 1e-6).all()


@pytest.mark.parametrize("representation", ["quaternion", "euler"])
def test_quadx_waypoints_with_yaw_targets(pts, representation):
    eng, obs, p, q, v, w = one_step(pts, "quadx", "waypoints", representation, use_yaw_targets=True)
    assert specialised(eng)
    name = f"quadx-waypoints yaw {representation}"
    H = check_block(pts, name, obs, p, q, v, w, representation == "quaternion")
    check_waypoints(pts, name, eng, H, obs, p, representation == "quaternion")
    TA.print_ratios(name)


# ------------------------------------------------------------------------------------------------ MA-Hover, Rocket-Landing, Dogfight
@pytest.mark.parametrize("representation", ["quaternion", "euler"])
def test_ma_hover(pts, representation):
    def spawn(eng):  # the reference's four start positions, level (the per-lane spawn lives in the state's side block)
        pos = np.array([[-1, -1, 1], [1, -1, 1], [-1, 1, 1], [1, 1, 1]], f32)
        side = np.zeros((pts.n, 12), f32)
        side[:, :3] = np.tile(pos, (pts.n // 4, 1))
        side[:, 6] = 1.0
        eng.state[12:15] = torch.tensor(side, device=DEV).view(pts.n, 3, 4).permute(1, 0, 2)

    eng, obs, p, q, v, w = one_step(pts, "quadx", "ma_hover", representation, setup=spawn)
    print(f"\nMA-Hover runs the {'specialised' if specialised(eng) else 'generic'} kernel")
    check_block(pts, f"ma-hover {representation}", obs, p, q, v, w, representation == "quaternion")
    TA.print_ratios(f"MA-Hover, {representation}")


@pytest.mark.parametrize("lanes", ["flying", "ended"])
@pytest.mark.parametrize("representation", ["quaternion", "euler"])
def test_rocket_landing(pts, representation, lanes):
    eng, obs, p, q, v, w = one_step(pts, "rocket", "rocket_landing", representation, reset_options=0, ended=FLAGS_GROUP["rocket"] if lanes == "ended" else None)
    if lanes == "ended":
        assert np.array_equal(q.astype(f32), pts.q)
    check_block(pts, f"rocket-landing {representation} {lanes}", obs, p, q, v, w, representation == "quaternion")
    TA.print_ratios(f"Rocket-Landing, {representation}, lanes {lanes}")


def test_dogfight_own_attitude_block(pts):
    def spawn(eng):  # pairs 100 m apart at 60 m, level (state groups 13 / 14: (x, y, z, roll), (pitch, yaw, -, -))
        g = torch.zeros(2, pts.n, 4, device=DEV)
        g[0, 0::2, 0] = 0.0
        g[0, 1::2, 0] = 100.0
        g[0, :, 2] = 60.0
        eng.state[13:15] = g

    eng, obs, p, q, v, w = one_step(pts, "fixedwing", "dogfight", "euler", setup=spawn, vehicle_options=dict(drone_model="acrowing"),
                                    world_options=dict(world_scale=5.0), dogfight=dict(team_size=1, sample_spawn=False))
    check_block(pts, "dogfight euler", obs, p, q, v, w, False, position=False)
    TA.print_ratios("Dogfight, own attitude block")


# ------------------------------------------------------------------------------------------------ the Aviary accessors
@pytest.mark.parametrize("vehicle", ["quadx", "fixedwing", "rocket"])
def test_aviary_states_at_the_attitude_set(pts, vehicle):
    """Aviary(pos, rpy, vehicle) at the attitude set given as Euler angles -- the ladder up to the gimbal threshold included, where
    test_gpu_kat.py's round trip stops at |pitch| = 1.5: all_states rows 0-2 (w_b, rpy, v_b) against the reference of the engine's
    read-back quaternion."""
    from pyflyt_amd.core import Aviary

    rpy = pts.designed.euler[: pts.att.n]
    pos = np.tile(np.array([[0.0, 0.0, 100.0]]), (len(rpy), 1))
    env = Aviary(pos, rpy, vehicle, motor_noise=False)
    st = env.all_states.double().cpu().numpy()
    p, q, v, w = base(env.engine)
    env.disconnect()
    H = Held(pts, q)
    tab = H.tab
    counts = [int((tab.bins == b).sum()) for b in range(R.N_BINS)]
    print(f"\nAviary {vehicle}: read-back attitudes per bin " + ", ".join(f"{n} {c}" for n, c in zip(R.BIN_NAMES, counts)) + f"; on a jump {int(tab.jump.sum())}")
    assert min(counts[1:6]) >= 200 and counts[R.GIMBAL_BIN] >= 64, counts
    TA.check_euler(H, f"aviary {vehicle} rpy", st[:, 1].astype(f32), True)
    BR = R.bound(0.0, TA.M_COMPOSITE, tab.e_R, tab.m_R)[tab.bins].max(1)
    R0 = tab.R.reshape(-1, 3, 3)
    for what, got, x in (("v_b", st[:, 2], v), ("w_b", st[:, 0], w)):
        bnd = (BR + 3 * EPS) * np.abs(x).sum(1) + 1e-45
        assert (np.abs(got - np.einsum("nji,nj->ni", R0, x)) <= bnd[:, None]).all(), (vehicle, what)
    assert np.array_equal(st[:, 3].astype(f32).view(np.uint32), p.astype(f32).view(np.uint32))
    TA.print_ratios(f"Aviary {vehicle}")

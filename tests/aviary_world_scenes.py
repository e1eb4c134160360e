"""Scenes for the shared-world Aviary tests (drones_per_world = K > 1), on the fp64 oracle: W worlds of K drones, each world stepped
by orc_world_aviary_step through pointer arrays built the way oracle.OracleWorld builds them. QuadX drones fly in flight mode -1
(the setpoint is the motor command, no controller), so that what the world couples -- pair impulses, the world-wide drag gate of
quadx.py:509 -- shows in the state without a controller answering it. Imported by tests/test_cpu_aviary_world.py and
tests/test_gpu_aviary_world.py."""
import ctypes as C

import numpy as np

from oracle import oracle as O

PWM_FLY = 0.7  # a little under the cf2x hover command (thrust-to-weight 2: pwm 0.707)
SPIN = 6.0     # rad/s about the body z axis: what the rotational drag (drag_coef_pqr 1e-4 / Izz 2.17e-5) acts on


def scene(name, K, W, vehicle="quadx"):
    """start positions [W*K, 3], start orientations, start velocities, angular velocities (world frame) and setpoints [W*K, 4 | 6]."""
    n = W * K
    pos, orn, vel, ang = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    sp = np.full((n, 4), PWM_FLY) if vehicle == "quadx" else np.tile([0.0, 0.0, 0.0, 0.6, 0.0, 0.0], (n, 1))[:, :4]
    for w in range(W):
        base = np.array([20.0 * w, 0.0, 0.0])  # (worlds are apart on the device anyway; here it keeps the scenes readable)
        for i in range(K):
            r = w * K + i
            pos[r] = base + [0.0, 2.0 * i, 1.5 + 0.1 * (i % 3)]
            ang[r] = [0.0, 0.0, 0.5 * (i + 1) * (-1) ** i]
        if name == "converging":  # drones 0 and 1 on a head-on course, 0.4 m apart closing at 2 m/s, slightly offset
            pos[w * K + 0] = base + [-0.2, 0.0, 1.0]
            pos[w * K + 1] = base + [0.2, 0.01 * w, 1.01]
            vel[w * K + 0] = [1.0, 0.0, 0.0]
            vel[w * K + 1] = [-1.0, 0.0, 0.0]
        elif name == "landing":  # drone 0 drops from 0.3 m with the motors off; the others fly with a spin
            pos[w * K + 0] = base + [0.0, -1.0, 0.3 + 0.02 * w]
            orn[w * K + 0] = [0.05, -0.03, 0.0]
            ang[w * K + 0] = 0.0
            if vehicle == "quadx":
                sp[w * K + 0] = 0.0
            for i in range(1, K):
                ang[w * K + i] = [0.0, 0.0, SPIN * (1.0 + 0.1 * i)]
        elif name != "apart":
            raise ValueError(name)
    if vehicle == "fixedwing":  # aeroplanes (1.5 m of fuselage behind the base origin, 2.2 m of wing): wider, higher, faster
        ang[:] = 0.0
        pos[:, 1] *= 2.0
        pos[:, 2] += 4.0
        if name == "converging":
            for w in range(W):
                pos[w * K + 0, 0], pos[w * K + 1, 0] = 20.0 * w - 1.5, 20.0 * w + 1.5
                vel[w * K + 0], vel[w * K + 1] = [3.0, 0.0, 0.0], [-3.0, 0.0, 0.0]
    return pos, orn, vel, ang, sp


class OracleAviaryWorlds:
    """W worlds of K drones on the oracle, reset like Aviary.reset + set_mode + set_all_setpoints, then given the scene's velocities."""

    def __init__(self, vehicle, K, W, pos, orn, vel, ang, sp, mode):
        lib = self.lib = O.lib()
        self.K, self.W, self.n = K, W, K * W
        self.lanes = (O.Lane * self.n)()  # (the attribute pack_state reads)
        pos32 = pos.astype(np.float32).astype(np.float64)  # the device spawns at the float32 pose
        extra = dict(start_vel=[0.0, 0.0, 0.0]) if vehicle == "fixedwing" else {}
        self.Ps = [O.make_params(vehicle, noise_mode=O.NOISE_OFF, start_pos=pos32[i], start_rpy=orn[i], **extra) for i in range(self.n)]
        for i in range(self.n):
            L = self.lanes[i]
            lib.orc_aviary_reset(C.byref(self.Ps[i]), C.byref(L), i)
            lib.orc_set_mode(C.byref(self.Ps[i]), C.byref(L), mode)
            for j in range(8):
                L.setpoint[j] = float(sp[i][j]) if j < sp.shape[1] else 0.0
            for k in range(3):
                L.v[k] = float(np.float32(vel[i][k]))
                L.w[k] = float(np.float32(ang[i][k]))
            lib.orc_update_state(C.byref(self.Ps[i]), C.byref(L))
        PP, LP = C.POINTER(O.Params), C.POINTER(O.Lane)
        self._pp = [(PP * K)(*[C.pointer(self.Ps[w * K + i]) for i in range(K)]) for w in range(W)]
        self._lp = [(LP * K)(*[C.pointer(self.lanes[w * K + i]) for i in range(K)]) for w in range(W)]
        # the same drones, each alone in a world of its own (what drones_per_world=1 computes)
        self._pp1 = [(PP * 1)(C.pointer(self.Ps[i])) for i in range(self.n)]
        self._lp1 = [(LP * 1)(C.pointer(self.lanes[i])) for i in range(self.n)]

    def step(self, solo=False):
        if solo:
            for i in range(self.n):
                self.lib.orc_world_aviary_step(self._pp1[i], self._lp1[i], 1, None, 0, 0)
        else:
            for w in range(self.W):
                self.lib.orc_world_aviary_step(self._pp[w], self._lp[w], self.K, None, 0, 0)

    def states(self):
        """[n, 4, 3]: ang_vel, ang_pos, lin_vel (body frame), lin_pos -- Aviary.all_states' rows."""
        return np.array([[list(L.w_b), list(L.rpy), list(L.v_b), list(L.p)] for L in self.lanes])

    def contact_step(self):
        return np.array([bool(L.contact_step) for L in self.lanes])

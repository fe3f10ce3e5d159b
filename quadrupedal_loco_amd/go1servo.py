"""Batched Go1 servo tick (fp64) on gfx950: joint state, IMU quaternion and
the /MPC/Gait row in; joint commands, joint torques and the
/control2rtmpc/state row out.

Python mirror of one iteration of the sim servo loop
(unitree_ros/go1_rt_control/src/servo_control/servo.cpp:675-1330, and the
go1_gait_data row of :1333-1433) for B robots started together -- include/qloco.h
section 16, csrc/qloco_go1_servo.hip:

  Go1ServoTick.step   quat_to_euler and Forward_kinematics_g x 4, the measured
                      foot velocity, the state row, then the stand-up branch or
                      the gait branch (counters, 15 Butterworth filters, per-mode
                      targets, Inverse_kinematics_g x 4, the force block's glue)
                      in one kernel, followed on the same stream by the force QP
                      and compute_joint_torques -- no host step in between.

All member state (filter memories, angle_des, the homing feet, targets, the
_old / _pre sets, counters, swing flags, F_leg_ref, grf_opt, Legs_torque) lives
in a device workspace; `n_count`, the node's loop counter, is kept by the
object.  There is no host fallback.  Legs are FR, FL, RR, RL; 3x3 matrices are
column-major.
"""
import ctypes as C

import numpy as np

from ._lib import GO1_SERVO_DIAG, Go1ServoDiag, Go1ServoParams, check, lib, ptr
from ._rows import rows_arg
from .qp import FORCE_BODY_LEN, _stream

STATE = 288           # QLOCO_GO1_SERVO_STATE
GAIT_DATA_LEN = 100   # QLOCO_GO1_GAIT_DATA_LEN
FILTERS = 15          # QLOCO_GO1_SERVO_FILTERS
# gait slot each filter reads, in the loop's order (servo.cpp:898-931)
FILTER_SLOTS = (0, 1, 2, 9, 10, 11, 6, 7, 8, 39, 40, 41, 73, 74, 75)
STATE_FIELDS = dict(  # slices of the dense record get_state / set_state use
    filters=(0, 75), angle_des=(75, 87), foot_homing=(87, 99), body_p_homing=(99, 102),
    body_p_des=(102, 105), body_r_des=(105, 108), foot_des=(108, 120),
    foot_rel_des_old=(120, 132), foot_rel_mea_old=(132, 144), com_des_pre=(144, 147),
    v_relative=(147, 159), v_est_rel=(159, 171), count_in_rt_loop=(171, 172), swing=(172, 176),
    F_leg_ref=(176, 188), grf_opt=(188, 200), Legs_torque=(200, 212), com_des=(212, 215),
    rfoot_des=(215, 218), lfoot_des=(218, 221), coma_des=(221, 224), thetaacc_des=(224, 227),
    comv_des=(227, 230), t_int=(230, 231), Force_L_R=(231, 237), F_sum=(237, 243), Jaco=(243, 279),
    qp_solution=(279, 280), status=(280, 281))
TARGET_POS = (0.0, 0.87, -1.5) * 4   # servo.cpp:767


def default_params(**overrides):
    """servo.cpp's constants (include/qloco.h section 16); `force` takes a dict
    of qloco_force_params fields, `target_pos` a sequence of 12."""
    p = Go1ServoParams()
    lib().qloco_go1_servo_params_default(C.byref(p))
    for k, v in overrides.items():
        if k == "force":
            for fk, fv in v.items():
                setattr(p.force, fk, fv)
        elif k == "target_pos":
            if len(v) != 12:
                raise ValueError("target_pos: 12 values expected")
            for i, x in enumerate(v):
                p.target_pos[i] = x
        elif k in ("filter", "reserved") or not hasattr(p, k):
            raise ValueError("unknown parameter %r" % k)
        else:
            setattr(p, k, v)
    return p


class Go1ServoResult:
    """Outputs of one tick (device tensors owned by the Go1ServoTick and
    overwritten by the next step): q_cmd, ctrl_msg, tau, grf_opt, gait_data
    (or None) and every member of qloco_go1_servo_diag by name."""

    def __init__(self, tensors, homing, n_count):
        self.__dict__.update(tensors)
        self.homing = homing
        self.n_count = n_count


class Go1ServoTick:
    """One servo node per robot, B robots started together."""

    def __init__(self, batch, device="cuda:0", gait_data=False, diag=True, **params):
        import torch
        self.batch = int(batch)
        self.device = torch.device(device)
        self.params = default_params(**params)
        self.n_count = 0
        n = int(lib().qloco_go1_servo_workspace_bytes(self.batch))
        if n < 0:
            raise ValueError("batch must be positive")
        self.ws = torch.empty(n, dtype=torch.uint8, device=self.device)
        f64 = dict(dtype=torch.float64, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        B = self.batch
        self.out = {"q_cmd": torch.zeros((B, 12), **f64), "ctrl_msg": torch.zeros((B, 25), **f64),
                    "tau": torch.zeros((B, 12), **f64), "grf_opt": torch.zeros((B, 12), **f64),
                    "gait_data": torch.zeros((B, GAIT_DATA_LEN), **f64) if gait_data else None}
        self.diag = Go1ServoDiag() if diag else None   # diag=False: none of the optional members is written
        for name, n_, kind in GO1_SERVO_DIAG if diag else ():
            shape = (B, n_) if n_ > 1 else (B,)
            t = torch.zeros(shape, **(f64 if kind == "f8" else i32))
            self.out[name] = t
            setattr(self.diag, name, t.data_ptr())
        check(lib().qloco_go1_servo_init(C.byref(self.params), B, ptr(self.ws), _stream(self.ws)),
              "qloco_go1_servo_init")

    def _in(self, t, name, cols, dtype):
        if t.dtype != dtype or not t.is_cuda:
            raise ValueError("%s: need a %s device tensor" % (name, dtype))
        t = t.contiguous()
        if t.numel() != self.batch * cols:
            raise ValueError("%s: need %d values per robot" % (name, cols))
        return t

    def homing(self, n_count=None):
        """The branch of servo.cpp:769 at this n_count."""
        n = self.n_count if n_count is None else n_count
        p = self.params
        return n * (1.0 / p.rt_frequency) <= p.stand_duration

    def step(self, q_mea, quat, gait_msg, gait_mode, y_offset, body=None):
        """One loop iteration; increments n_count.  body: (B, 16) float64
        device rows of qp.force_body_rows, one per robot, read by the gait
        branch only."""
        import torch
        q_mea = self._in(q_mea, "q_mea", 12, torch.float64)
        quat = self._in(quat, "quat", 4, torch.float64)
        gait_msg = self._in(gait_msg, "gait_msg", 100, torch.float64)
        gait_mode = self._in(gait_mode, "gait_mode", 1, torch.int32)
        y_offset = self._in(y_offset, "y_offset", 1, torch.float64)
        o = self.out
        body = rows_arg(body, self.batch, FORCE_BODY_LEN, torch.float64, o["tau"].device)
        homing = self.homing()
        check(lib().qloco_go1_servo_tick_body(
            C.byref(self.params), self.batch, ptr(self.ws), self.n_count, ptr(q_mea), ptr(quat),
            ptr(gait_msg), ptr(gait_mode), ptr(y_offset), ptr(o["q_cmd"]), ptr(o["ctrl_msg"]),
            ptr(o["tau"]), ptr(o["grf_opt"]), C.byref(self.diag) if self.diag else None, ptr(o["gait_data"]),
            ptr(body), _stream(self.ws)), "qloco_go1_servo_tick_body")
        res = Go1ServoResult(o, homing, self.n_count)
        self.n_count += 1
        return res

    def get_state(self):
        """(B, STATE) float64 device tensor: the dense per-robot record."""
        import torch
        s = torch.empty((self.batch, STATE), dtype=torch.float64, device=self.device)
        check(lib().qloco_go1_servo_get_state(self.batch, ptr(self.ws), ptr(s), _stream(self.ws)),
              "qloco_go1_servo_get_state")
        return s

    def set_state(self, state, n_count=None):
        import torch
        state = self._in(state, "state", STATE, torch.float64)
        check(lib().qloco_go1_servo_set_state(self.batch, ptr(self.ws), ptr(state),
                                              _stream(self.ws)), "qloco_go1_servo_set_state")
        if n_count is not None:
            self.n_count = int(n_count)


def _robot_mode(r):
    """Gait mode of robot r: 102, 101, 103 in turn, robot 3 alone outside them."""
    return 100 if r == 3 else (102, 101, 103)[r % 3]


def synth_inputs(seed, batch, ticks, n_t_int=5, first_robot=0):
    """Deterministic open-loop inputs, a pure function of (seed, robot, tick):
    the measured joints do not depend on the commands.  Returns numpy arrays
    q_mea (T, B, 12) within +-0.15 rad of the target pose, quat (T, B, 4)
    normalised with |roll|, |pitch| <= 0.3 rad, gait_msg (T, B, 100) held for
    n_t_int ticks (CoM advancing, |coma| <= 2 m/s^2, feet y centred on
    -+0.12675, x offsets <= 0.08 m, lift <= 0.05 m, right_support cycling
    through 0 / 1 / 2), gait_mode (B,) and y_offset (B,)."""
    T, B = int(ticks), int(batch)
    q = np.zeros((T, B, 12))
    quat = np.zeros((T, B, 4))
    gait = np.zeros((T, B, 100))
    mode = np.zeros(B, np.int32)
    yoff = np.zeros(B)
    tk = np.arange(T)
    g = tk // n_t_int                     # index of the gait row a tick sees
    tg = g * 0.025
    for b in range(B):
        r = first_robot + b
        rng = np.random.default_rng([seed, r])
        ph = rng.uniform(0, 2 * np.pi, 16)
        amp = rng.uniform(0.03, 0.1, 12)
        mode[b] = _robot_mode(r)
        yoff[b] = {101: 0.75, 102: 0.0}.get(int(mode[b]), 0.11)
        t = tk * 0.001
        noise = np.stack([np.random.default_rng([seed, r, int(k)]).uniform(-0.04, 0.04, 12) for k in tk])
        q[:, b] = np.asarray(TARGET_POS) + amp * np.sin(2 * np.pi * 3 * t[:, None] + ph[:12]) + noise
        roll = 0.25 * np.sin(2 * np.pi * 2 * t + ph[12])
        pitch = 0.25 * np.sin(2 * np.pi * 1.5 * t + ph[13])
        yaw = 0.8 * np.sin(2 * np.pi * 0.7 * t + ph[14])
        cr, sr, cp, sp, cy, sy = (np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2),
                                  np.cos(yaw / 2), np.sin(yaw / 2))
        qq = np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy,
                       cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], 1)
        quat[:, b] = qq / np.linalg.norm(qq, axis=1, keepdims=True)
        # the /MPC/Gait row
        cx = 0.08 * tg + 0.004 * np.sin(4 * tg + ph[0])
        cyy = 0.01 * np.sin(5 * tg + ph[1])
        cz = 0.29 + 0.004 * np.cos(6 * tg + ph[2])
        gait[:, b, 0], gait[:, b, 1], gait[:, b, 2] = cx, cyy, cz
        s = np.sin(2 * np.pi * tg / 0.35 + ph[3])
        gait[:, b, 9] = cx + 0.06 * s
        gait[:, b, 10] = -0.12675 + 0.01 * np.sin(3 * tg + ph[4])
        gait[:, b, 11] = 0.05 * np.maximum(s, 0.0) ** 2
        gait[:, b, 6] = cx - 0.06 * s
        gait[:, b, 7] = 0.12675 + 0.01 * np.sin(3 * tg + ph[5])
        gait[:, b, 8] = 0.05 * np.maximum(-s, 0.0) ** 2
        for k in range(3):
            gait[:, b, 39 + k] = 1.5 * np.sin(7 * tg + ph[6 + k])
            gait[:, b, 73 + k] = 0.5 * np.sin(9 * tg + ph[9 + k])
        gait[:, b, 27] = 1 + g // 7
        gait[:, b, 99] = (g // 3 + r) % 3
    return dict(q_mea=q, quat=quat, gait_msg=gait, gait_mode=mode, y_offset=yoff)

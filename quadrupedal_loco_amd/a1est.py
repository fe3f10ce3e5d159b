"""Batched A1 state estimation front end (fp64) on gfx950.

Python mirror of the input side of the A1 control loop
(unitree_ros/a1_cpp_open_source/src):

  A1LegKin     the per-leg block of GazeboA1ROS::gt_pose_callback
               (GazeboA1ROS.cpp:306-331): A1Kinematics::fk / jac, foot
               velocities, root_rot_mat / root_euler / root_rot_mat_z and the
               body / world frame foot arrays -- `qloco_a1_leg_kin`.
  A1Estimator  A1BasicEKF (A1BasicEKF.cpp:55-164) as main_update calls it
               (GazeboA1ROS.cpp:204-209): init_state, then update_estimation
               once per tick, filter state resident in a device workspace --
               `qloco_a1_ekf_*`.

Legs are FL, FR, RL, RR; 3x3 and 3x4 matrices are column-major, so the
outputs can fill the a1qp state record's [0:3], [6:9], [12:15], [24:33],
[33:42] and [42:54] fields.  The compute is csrc/qloco_a1est.hip; there is no
host fallback.  The IMU moving-window filters (GazeboA1ROS.cpp:334-349) stay
with the caller.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._lib import A1EkfParams, A1KinParams, check, lib, ptr

NX = 18   # STATE_SIZE
NY = 28   # MEAS_SIZE
STAND_Q = (0.0, 0.72, -1.44)  # hip, thigh, calf: feet about 0.32 m below the hips


def default_kin_params():
    """rho_fix / rho_opt of GazeboA1ROS.cpp:79-101."""
    p = A1KinParams()
    lib().qloco_a1_kin_params_default(C.byref(p))
    return p


def default_ekf_params(**overrides):
    """The A1BasicEKF.h:16-21 noise constants, assume_flat_ground = 1."""
    p = A1EkfParams()
    lib().qloco_a1_ekf_params_default(C.byref(p))
    for k, v in overrides.items():
        setattr(p, k, v)
    return p


def _dev(t, dtype, shape, name):
    import torch
    want = {"f64": torch.float64, "i32": torch.int32, "u8": torch.uint8}[dtype]
    if t.dtype != want or not t.is_contiguous() or not t.is_cuda or tuple(t.shape) != tuple(shape):
        raise ValueError("%s: contiguous %s %s device tensor expected" % (name, dtype, tuple(shape)))
    return t


@dataclass
class A1KinResult:
    foot_pos_rel: object      # (B, 12), 3x4 col-major
    j_foot: object            # (B, 36): four 3x3 col-major diagonal blocks
    foot_vel_rel: object      # (B, 12)
    root_rot_mat: object      # (B, 9)
    root_euler: object        # (B, 3) roll, pitch, yaw
    root_rot_mat_z: object    # (B, 9)
    foot_pos_abs: object      # (B, 12)
    foot_vel_abs: object      # (B, 12)
    foot_pos_world: object = None
    foot_vel_world: object = None


class A1LegKin:
    """Batched drop-in for the per-leg block of gt_pose_callback."""

    def __init__(self, params=None):
        self.params = params if params is not None else default_kin_params()

    def forward(self, joint_pos, joint_vel, root_quat, root_pos=None, root_lin_vel=None,
                out=None, stream=None):
        import torch
        B = joint_pos.shape[0]
        _dev(joint_pos, "f64", (B, 12), "joint_pos")
        _dev(joint_vel, "f64", (B, 12), "joint_vel")
        _dev(root_quat, "f64", (B, 4), "root_quat")
        if root_pos is not None:
            _dev(root_pos, "f64", (B, 3), "root_pos")
        if root_lin_vel is not None:
            _dev(root_lin_vel, "f64", (B, 3), "root_lin_vel")
        dev = joint_pos.device
        if out is None:
            e = lambda n: torch.empty((B, n), dtype=torch.float64, device=dev)
            out = A1KinResult(e(12), e(36), e(12), e(9), e(3), e(9), e(12), e(12))
            if root_pos is not None:
                out.foot_pos_world = e(12)
            if root_lin_vel is not None:
                out.foot_vel_world = e(12)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        check(lib().qloco_a1_leg_kin(
            C.byref(self.params), B, ptr(joint_pos), ptr(joint_vel), ptr(root_quat),
            ptr(root_pos), ptr(root_lin_vel), ptr(out.foot_pos_rel), ptr(out.j_foot),
            ptr(out.foot_vel_rel), ptr(out.root_rot_mat), ptr(out.root_euler),
            ptr(out.root_rot_mat_z), ptr(out.foot_pos_abs), ptr(out.foot_vel_abs),
            ptr(out.foot_pos_world), ptr(out.foot_vel_world), C.c_void_p(stream)),
            "qloco_a1_leg_kin")
        return out


@dataclass
class A1EstResult:
    root_pos: object            # (B, 3) = x[0:3]
    root_lin_vel: object        # (B, 3) = x[3:6]
    estimated_contacts: object  # (B, 4) uint8


class A1Estimator:
    """Batched drop-in for A1BasicEKF; one filter per robot, state on the device."""

    def __init__(self, batch, device, params=None, **overrides):
        import torch
        if batch < 1:
            raise ValueError("batch < 1")
        self.batch = int(batch)
        self.device = torch.device(device)
        self.params = params if params is not None else default_ekf_params(**overrides)
        nbytes = lib().qloco_a1_ekf_workspace_bytes(self.batch)
        if nbytes <= 0:
            raise ValueError("qloco_a1_ekf_workspace_bytes(%d) = %d" % (self.batch, nbytes))
        self.workspace = torch.zeros(nbytes // 8, dtype=torch.float64, device=self.device)
        self.inited = False

    def is_inited(self):
        return self.inited

    def _stream(self, stream):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream
                          if stream is None else stream)

    def init(self, root_rot_mat, foot_pos_rel, stream=None):
        B = self.batch
        _dev(root_rot_mat, "f64", (B, 9), "root_rot_mat")
        _dev(foot_pos_rel, "f64", (B, 12), "foot_pos_rel")
        check(lib().qloco_a1_ekf_init(C.byref(self.params), B, ptr(self.workspace),
                                      ptr(root_rot_mat), ptr(foot_pos_rel), self._stream(stream)),
              "qloco_a1_ekf_init")
        self.inited = True

    def update(self, dt, movement_mode, root_rot_mat, imu_acc, imu_ang_vel, foot_pos_rel,
               foot_vel_rel, foot_force, out=None, stream=None):
        import torch
        B = self.batch
        _dev(dt, "f64", (B,), "dt")
        _dev(movement_mode, "i32", (B,), "movement_mode")
        _dev(root_rot_mat, "f64", (B, 9), "root_rot_mat")
        _dev(imu_acc, "f64", (B, 3), "imu_acc")
        _dev(imu_ang_vel, "f64", (B, 3), "imu_ang_vel")
        _dev(foot_pos_rel, "f64", (B, 12), "foot_pos_rel")
        _dev(foot_vel_rel, "f64", (B, 12), "foot_vel_rel")
        _dev(foot_force, "f64", (B, 4), "foot_force")
        if out is None:
            out = A1EstResult(torch.empty((B, 3), dtype=torch.float64, device=self.device),
                              torch.empty((B, 3), dtype=torch.float64, device=self.device),
                              torch.empty((B, 4), dtype=torch.uint8, device=self.device))
        check(lib().qloco_a1_ekf_update(
            C.byref(self.params), B, ptr(self.workspace), ptr(dt), ptr(movement_mode),
            ptr(root_rot_mat), ptr(imu_acc), ptr(imu_ang_vel), ptr(foot_pos_rel),
            ptr(foot_vel_rel), ptr(foot_force), ptr(out.root_pos), ptr(out.root_lin_vel),
            ptr(out.estimated_contacts), self._stream(stream)), "qloco_a1_ekf_update")
        return out

    def state(self, stream=None):
        """Dense (x (B, 18), P (B, 18, 18)); P is symmetric, so its memory order is moot."""
        import torch
        B = self.batch
        x = torch.empty((B, NX), dtype=torch.float64, device=self.device)
        P = torch.empty((B, NX, NX), dtype=torch.float64, device=self.device)
        check(lib().qloco_a1_ekf_get_state(B, ptr(self.workspace), ptr(x), ptr(P),
                                           self._stream(stream)), "qloco_a1_ekf_get_state")
        return x, P

    def load_state(self, x, P, stream=None):
        """x (B, 18), P (B, 18, 18) taken as column-major per robot: entry
        (i, j), i >= j, is read from P[b, j, i]."""
        B = self.batch
        _dev(x, "f64", (B, NX), "x")
        _dev(P, "f64", (B, NX, NX), "P")
        check(lib().qloco_a1_ekf_set_state(B, ptr(self.workspace), ptr(x), ptr(P),
                                           self._stream(stream)), "qloco_a1_ekf_set_state")
        self.inited = True


# ---------------------------------------------------------------- host generator
def quat_to_rot(q):
    """Eigen Quaternion::toRotationMatrix for q = (w, x, y, z) rows -> (..., 3, 3)."""
    w, x, y, z = (q[..., k] for k in range(4))
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0] = 1.0 - (tyy + tzz)
    R[..., 0, 1] = txy - twz
    R[..., 0, 2] = txz + twy
    R[..., 1, 0] = txy + twz
    R[..., 1, 1] = 1.0 - (txx + tzz)
    R[..., 1, 2] = tyz - twx
    R[..., 2, 0] = txz - twy
    R[..., 2, 1] = tyz + twx
    R[..., 2, 2] = 1.0 - (txx + tyy)
    return R


def chain_fk(q, qd, rho_fix):
    """A1 leg kinematics from the kinematic chain (rho_opt = 0), numpy, host:
    q, qd (..., 4, 3), rho_fix (4, 5) -> foot position, J (row, col) and J qd.
    Equal to the generated closed forms in real arithmetic; used by
    synth_inputs, not by the device path."""
    ox, oy, d, lu, ll = (rho_fix[:, k] for k in range(5))
    s0, c0 = np.sin(q[..., 0]), np.cos(q[..., 0])
    s1, c1 = np.sin(q[..., 1]), np.cos(q[..., 1])
    s12, c12 = np.sin(q[..., 1] + q[..., 2]), np.cos(q[..., 1] + q[..., 2])
    L = lu * c1 + ll * c12
    S = lu * s1 + ll * s12
    p = np.stack([ox - S, oy + d * c0 + s0 * L, d * s0 - c0 * L], -1)
    J = np.zeros(q.shape[:-1] + (3, 3))
    J[..., 1, 0] = -d * s0 + c0 * L
    J[..., 2, 0] = d * c0 + s0 * L
    J[..., 0, 1] = -L
    J[..., 1, 1] = -s0 * S
    J[..., 2, 1] = c0 * S
    J[..., 0, 2] = -ll * c12
    J[..., 1, 2] = -s0 * ll * s12
    J[..., 2, 2] = c0 * ll * s12
    return p, J, np.einsum("...ij,...j->...i", J, qd)


def synth_inputs(seed, batch, ticks, dt=0.0025):
    """Deterministic synthetic A1 sensor streams (numpy, host), arrays (ticks,
    batch, ...): joint angles swinging around the stand pose with their rates,
    small roll / pitch and any yaw (root_quat as w, x, y, z), imu_acc near
    R'(a + g) and imu_ang_vel, a trot's foot_force -- stance ~ U(60, 140),
    swing ~ U(-5, 20), so both clamp ends of the contact estimate and its 0.5
    threshold are crossed -- and movement_mode (batch,), 0 for every fourth
    robot.  The derived estimator inputs (root_rot_mat, foot_pos_rel,
    foot_vel_rel, host arithmetic) ride along for host-side checkers."""
    rng = np.random.default_rng(seed)
    T, B = ticks, batch
    t = (np.arange(T) * dt)[:, None]
    kp = default_kin_params()
    rho_fix = np.array([[kp.rho_fix[l][k] for k in range(5)] for l in range(4)])
    # joints: stand pose + per-joint sinusoid
    amp = rng.uniform(0.02, 0.25, (B, 12))
    frq = rng.uniform(0.5, 3.0, (B, 12)) * 2 * np.pi
    ph = rng.uniform(0, 2 * np.pi, (B, 12))
    q0 = np.tile(np.array(STAND_Q), 4)[None] + rng.uniform(-0.05, 0.05, (B, 12))
    joint_pos = q0[None] + amp[None] * np.sin(frq[None] * t[..., None] + ph[None])
    joint_vel = amp[None] * frq[None] * np.cos(frq[None] * t[..., None] + ph[None])
    # attitude: small roll / pitch oscillation, yaw anywhere and turning
    a_rp = rng.uniform(0.0, 0.1, (B, 2))
    f_rp = rng.uniform(0.5, 2.0, (B, 2)) * 2 * np.pi
    p_rp = rng.uniform(0, 2 * np.pi, (B, 2))
    roll = a_rp[None, :, 0] * np.sin(f_rp[None, :, 0] * t + p_rp[None, :, 0])
    pitch = a_rp[None, :, 1] * np.sin(f_rp[None, :, 1] * t + p_rp[None, :, 1])
    yaw = rng.uniform(-np.pi, np.pi, B)[None] + rng.uniform(-0.5, 0.5, B)[None] * t
    cr, sr, cp, sp, cy, sy = (np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2),
                              np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2))
    root_quat = np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy,
                          cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], -1)
    R = quat_to_rot(root_quat)
    # IMU: specific force R'(a + g) + noise, small body rates
    acc_w = rng.normal(0, 0.5, (T, B, 3)) + np.array([0.0, 0.0, 9.81])
    imu_acc = np.einsum("tbji,tbj->tbi", R, acc_w) + rng.normal(0, 0.05, (T, B, 3))
    imu_ang_vel = rng.normal(0, 0.3, (T, B, 3))
    # trot: diagonal pairs alternate every `period` ticks, per-robot phase
    period = rng.integers(8, 20, B)
    phase = rng.integers(0, 40, B)
    half = ((np.arange(T)[:, None] + phase[None]) // period[None]) % 2
    pair_a = np.array([1, 0, 0, 1])
    stance = np.where(half[..., None] == 0, pair_a, 1 - pair_a).astype(bool)
    both = rng.random((T, B, 1)) < 0.15          # double-support ticks
    stance = stance | both
    foot_force = np.where(stance, rng.uniform(60, 140, (T, B, 4)), rng.uniform(-5, 20, (T, B, 4)))
    movement_mode = np.where(np.arange(B) % 4 == 0, 0, 1).astype(np.int32)
    p, J, v = chain_fk(joint_pos.reshape(T, B, 4, 3), joint_vel.reshape(T, B, 4, 3), rho_fix)
    return dict(dt=np.full((T, B), dt), movement_mode=movement_mode, joint_pos=joint_pos,
                joint_vel=joint_vel, root_quat=root_quat, imu_acc=imu_acc,
                imu_ang_vel=imu_ang_vel, foot_force=foot_force,
                root_rot_mat=np.ascontiguousarray(R.transpose(0, 1, 3, 2)).reshape(T, B, 9),
                foot_pos_rel=p.reshape(T, B, 12), foot_vel_rel=v.reshape(T, B, 12))

"""Batched A1 gait plan, swing-leg control, terrain pitch and joint torques
(fp64) on gfx950.

Python mirror of the part of the A1 control loop that sits between the state
estimator and the force solver, and after the solver
(unitree_ros/a1_cpp_open_source/src/A1RobotControl.cpp):

  A1GaitSwing.plan_swing     update_plan then generate_swing_legs_ctrl
                             (:149-292, called back to back at
                             GazeboA1ROS.cpp:199-202) -- `qloco_a1_ctrl_plan_swing`
  A1GaitSwing.terrain        the stance_leg_control_type == 1 preamble of
                             compute_grf (:341-380, :604-620) -- `qloco_a1_ctrl_terrain`
  A1GaitSwing.joint_torques  compute_joint_torques (:294-324) --
                             `qloco_a1_ctrl_joint_torques`
  A1Tick                     one device-resident control tick: A1LegKin.forward,
                             plan_swing, A1Estimator.update, terrain, a
                             caller-supplied solver, joint_torques, all on one
                             stream (a linear chain: it captures into a graph
                             with no parallel branches)

The per-robot member state (gait counters, contact flags, foot targets, the
13 moving-window filters, the torque hold-off counter) lives in a device
workspace.  The compute is csrc/qloco_a1ctrl.hip; there is no host fallback.
Legs are FL, FR, RL, RR; 3x3 and 3x4 matrices are column-major.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import a1est
from ._lib import A1CtrlParams, check, lib, ptr
from .a1est import _dev

STATE = 958           # QLOCO_A1_CTRL_STATE
STATE_FIELDS = dict(  # slices of the dense record get_state / set_state use
    gait_counter=(0, 4), plan_contacts=(4, 8), early_contacts=(8, 12), contacts=(12, 16),
    foot_pos_start=(16, 28), foot_pos_rel_last_time=(28, 40), foot_pos_target_last_time=(40, 52),
    foot_pos_target_rel=(52, 64), foot_pos_recent_contact=(64, 76), foot_forces_kin=(76, 88),
    joint_torques=(88, 100), mpc_init_counter=(100, 101), terrain_pitch_angle=(101, 102),
    rc_fill=(102, 106), rc_head=(106, 110), rc_sum=(110, 122), rc_correction=(122, 134),
    terrain_fill=(134, 135), terrain_head=(135, 136), terrain_sum=(136, 137),
    terrain_correction=(137, 138), rc_ring=(138, 858), terrain_ring=(858, 958))


def default_params(**overrides):
    """A1CtrlStates::reset(), A1Params.h:38-45 and the A1RobotControl
    constructor's window lengths; array fields take sequences."""
    p = A1CtrlParams()
    lib().qloco_a1_ctrl_params_default(C.byref(p))
    for k, v in overrides.items():
        if hasattr(v, "__len__"):
            f = getattr(p, k)
            if len(v) != len(f):
                raise ValueError("%s: %d values expected" % (k, len(f)))
            for i, x in enumerate(v):
                f[i] = x
        else:
            setattr(p, k, v)
    return p


@dataclass
class A1PlanSwingResult:
    contacts: object                  # (B, 4) uint8: plan || early, the solvers' `contacts`
    plan_contacts: object             # (B, 4) uint8
    early_contacts: object            # (B, 4) uint8
    gait_counter: object              # (B, 4)
    foot_pos_target_rel: object       # (B, 12), 3x4 col-major
    foot_pos_target_abs: object       # (B, 12)
    foot_pos_target_world: object     # (B, 12)
    foot_pos_cur: object              # (B, 12)
    foot_forces_kin: object           # (B, 12)
    foot_pos_recent_contact: object   # (B, 12)


@dataclass
class A1TerrainResult:
    terrain_pitch_angle: object       # (B,)
    surf_coef: object                 # (B, 3) = (a1, a2, -1)
    root_euler_d: object              # (B, 3), entry 1 overwritten in place


class A1GaitSwing:
    """Batched drop-in for A1RobotControl's update_plan,
    generate_swing_legs_ctrl, terrain-pitch preamble and compute_joint_torques;
    one set of members per robot, resident on the device."""

    def __init__(self, batch, device, params=None, **overrides):
        import torch
        if batch < 1:
            raise ValueError("batch < 1")
        self.batch = int(batch)
        self.device = torch.device(device)
        self.params = params if params is not None else default_params(**overrides)
        nbytes = lib().qloco_a1_ctrl_workspace_bytes(self.batch)
        if nbytes <= 0:
            raise ValueError("qloco_a1_ctrl_workspace_bytes(%d) = %d" % (self.batch, nbytes))
        self.workspace = torch.zeros(nbytes // 8, dtype=torch.float64, device=self.device)
        self.reset()

    def _stream(self, stream):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream
                          if stream is None else stream)

    def _f64(self, *shape):
        import torch
        return torch.empty(shape, dtype=torch.float64, device=self.device)

    def reset(self, stream=None):
        check(lib().qloco_a1_ctrl_reset(C.byref(self.params), self.batch, ptr(self.workspace),
                                        self._stream(stream)), "qloco_a1_ctrl_reset")

    def plan_swing(self, dt, movement_mode, root_pos, root_lin_vel, root_lin_vel_d, root_rot_mat,
                   root_rot_mat_z, foot_pos_abs, foot_force, out=None, stream=None):
        import torch
        B = self.batch
        _dev(dt, "f64", (B,), "dt")
        _dev(movement_mode, "i32", (B,), "movement_mode")
        for name, t, n in (("root_pos", root_pos, 3), ("root_lin_vel", root_lin_vel, 3),
                           ("root_lin_vel_d", root_lin_vel_d, 3), ("root_rot_mat", root_rot_mat, 9),
                           ("root_rot_mat_z", root_rot_mat_z, 9), ("foot_pos_abs", foot_pos_abs, 12),
                           ("foot_force", foot_force, 4)):
            _dev(t, "f64", (B, n), name)
        if out is None:
            u8 = lambda: torch.empty((B, 4), dtype=torch.uint8, device=self.device)
            out = A1PlanSwingResult(u8(), u8(), u8(), self._f64(B, 4), *(self._f64(B, 12) for _ in range(6)))
        check(lib().qloco_a1_ctrl_plan_swing(
            C.byref(self.params), B, ptr(self.workspace), ptr(dt), ptr(movement_mode), ptr(root_pos),
            ptr(root_lin_vel), ptr(root_lin_vel_d), ptr(root_rot_mat), ptr(root_rot_mat_z),
            ptr(foot_pos_abs), ptr(foot_force), ptr(out.contacts), ptr(out.plan_contacts),
            ptr(out.early_contacts), ptr(out.gait_counter), ptr(out.foot_pos_target_rel),
            ptr(out.foot_pos_target_abs), ptr(out.foot_pos_target_world), ptr(out.foot_pos_cur),
            ptr(out.foot_forces_kin), ptr(out.foot_pos_recent_contact), self._stream(stream)),
            "qloco_a1_ctrl_plan_swing")
        return out

    def terrain(self, root_pos, root_euler_d, out=None, stream=None):
        """Overwrites root_euler_d[:, 1] in place."""
        B = self.batch
        _dev(root_pos, "f64", (B, 3), "root_pos")
        _dev(root_euler_d, "f64", (B, 3), "root_euler_d")
        if out is None:
            out = A1TerrainResult(self._f64(B), self._f64(B, 3), root_euler_d)
        out.root_euler_d = root_euler_d
        check(lib().qloco_a1_ctrl_terrain(
            C.byref(self.params), B, ptr(self.workspace), ptr(root_pos), ptr(root_euler_d),
            ptr(out.terrain_pitch_angle), ptr(out.surf_coef), self._stream(stream)),
            "qloco_a1_ctrl_terrain")
        return out

    def joint_torques(self, j_foot, foot_forces_grf, out=None, stream=None):
        B = self.batch
        _dev(j_foot, "f64", (B, 36), "j_foot")
        _dev(foot_forces_grf, "f64", (B, 12), "foot_forces_grf")
        if out is None:
            out = self._f64(B, 12)
        check(lib().qloco_a1_ctrl_joint_torques(
            C.byref(self.params), B, ptr(self.workspace), ptr(j_foot), ptr(foot_forces_grf), ptr(out),
            self._stream(stream)), "qloco_a1_ctrl_joint_torques")
        return out

    def get_state(self, stream=None):
        """Dense (B, 958) record per robot (STATE_FIELDS)."""
        s = self._f64(self.batch, STATE)
        check(lib().qloco_a1_ctrl_get_state(self.batch, ptr(self.workspace), ptr(s),
                                            self._stream(stream)), "qloco_a1_ctrl_get_state")
        return s

    def set_state(self, state, stream=None):
        _dev(state, "f64", (self.batch, STATE), "state")
        check(lib().qloco_a1_ctrl_set_state(self.batch, ptr(self.workspace), ptr(state),
                                            self._stream(stream)), "qloco_a1_ctrl_set_state")


# ------------------------------------------------------------------ whole tick
A1QP_STATE_LEN = 54   # QLOCO_A1_STATE_LEN, the section 9 state record


@dataclass
class A1TickResult:
    kin: object
    swing: object
    est: object
    terrain: object
    state: object            # (B, 54) section 9 record
    forces: object           # (B, 12) what the solver returned, or None
    joint_torques: object    # (B, 12), or None without a solver


class A1Tick:
    """One A1 control tick on the device, no host step between joint state and
    joint torques: leg kinematics -> plan + swing (from the previous tick's
    root estimate, as main_update does) -> EKF update -> terrain pitch ->
    `solver(state_record, contacts)` -> joint torques.  Every call goes to the
    same stream in that order.  `solver` returns body-frame forces (B, 12),
    e.g. lambda s, c: a1qp.A1QpBatch().solve(s, c).forces; with solver=None the chain stops after the
    terrain call and the torques use `foot_forces_grf` if given.  A fleet with per-robot bodies
    passes its rows (a1qp.body_rows, on the device) through the same callable:
    solver=lambda s, c: qp.solve(s, c, body=rows, stats=False).forces."""

    def __init__(self, batch, device, solver=None, use_terrain=True, kin=None, ctrl=None, est=None):
        import torch
        self.batch, self.device = int(batch), torch.device(device)
        self.kin = kin or a1est.A1LegKin()
        self.ctrl = ctrl or A1GaitSwing(batch, device)
        self.est = est or a1est.A1Estimator(batch, device)
        self.solver, self.use_terrain = solver, use_terrain
        z = lambda n: torch.zeros((self.batch, n), dtype=torch.float64, device=self.device)
        self.root_pos, self.root_lin_vel = z(3), z(3)     # the estimate, fed back tick to tick
        self.state = z(A1QP_STATE_LEN)
        self.out = None

    def step(self, dt, movement_mode, joint_pos, joint_vel, root_quat, imu_acc, imu_ang_vel, foot_force,
             root_lin_vel_d, root_euler_d, root_pos_d=None, root_ang_vel=None, root_ang_vel_d=None,
             foot_forces_grf=None):
        """Device tensors as the underlying calls take them; root_euler_d[:, 1]
        is overwritten by the terrain call.  Returns A1TickResult (buffers are
        reused from call to call, so a captured graph replays into them)."""
        o = self.out
        kin = self.kin.forward(joint_pos, joint_vel, root_quat, out=o.kin if o else None)
        swing = self.ctrl.plan_swing(dt, movement_mode, self.root_pos, self.root_lin_vel, root_lin_vel_d,
                                     kin.root_rot_mat, kin.root_rot_mat_z, kin.foot_pos_abs, foot_force,
                                     out=o.swing if o else None)
        if not self.est.is_inited():
            self.est.init(kin.root_rot_mat, kin.foot_pos_rel)
        est = self.est.update(dt, movement_mode, kin.root_rot_mat, imu_acc, imu_ang_vel, kin.foot_pos_rel,
                              kin.foot_vel_rel, foot_force, out=o.est if o else None)
        self.root_pos.copy_(est.root_pos)
        self.root_lin_vel.copy_(est.root_lin_vel)
        ter = None
        if self.use_terrain:
            ter = self.ctrl.terrain(self.root_pos, root_euler_d, out=o.terrain if o else None)
        # the section 9 record: root_pos | root_pos_d | root_euler | root_euler_d | root_lin_vel |
        # root_lin_vel_d | root_ang_vel | root_ang_vel_d | root_rot_mat | root_rot_mat_z | foot_pos_abs
        s = self.state
        s[:, 0:3].copy_(self.root_pos)
        if root_pos_d is not None:
            s[:, 3:6].copy_(root_pos_d)
        s[:, 6:9].copy_(kin.root_euler)
        s[:, 9:12].copy_(root_euler_d)
        s[:, 12:15].copy_(self.root_lin_vel)
        s[:, 15:18].copy_(root_lin_vel_d)
        if root_ang_vel is not None:
            s[:, 18:21].copy_(root_ang_vel)
        if root_ang_vel_d is not None:
            s[:, 21:24].copy_(root_ang_vel_d)
        s[:, 24:33].copy_(kin.root_rot_mat)
        s[:, 33:42].copy_(kin.root_rot_mat_z)
        s[:, 42:54].copy_(kin.foot_pos_abs)
        forces = foot_forces_grf
        if self.solver is not None:
            forces = self.solver(s, swing.contacts)
        tau = None
        if forces is not None:
            tau = self.ctrl.joint_torques(kin.j_foot, forces, out=o.joint_torques if o else None)
        self.out = A1TickResult(kin, swing, est, ter, s, forces, tau)
        return self.out


# ---------------------------------------------------------------- host generator
def synth_inputs(seed, batch, ticks, dt=0.0025):
    """Deterministic synthetic inputs of the three calls (numpy, host), arrays
    (ticks, batch, ...): a1est.synth_inputs' joint angles (stand pose plus
    sinusoids, inside the box tests/golden/make_a1_kin_golden.py draws from)
    and attitudes give root_rot_mat, root_rot_mat_z, foot_pos_abs and j_foot
    (host arithmetic); root_pos drifts around 0.28 m height; root_lin_vel and
    root_lin_vel_d are large enough that the Raibert offsets reach the +-0.1
    clamp on some robots; foot_force ~ U(-5, 60) straddles FOOT_FORCE_LOW;
    foot_forces_grf are plausible body-frame stance forces; movement_mode
    (ticks, batch) is 0 for every fourth robot."""
    e = a1est.synth_inputs(seed, batch, ticks, dt)
    rng = np.random.default_rng(seed + 50000)
    T, B = ticks, batch
    kp = a1est.default_kin_params()
    rho_fix = np.array([[kp.rho_fix[l][k] for k in range(5)] for l in range(4)])
    p, J, _ = a1est.chain_fk(e["joint_pos"].reshape(T, B, 4, 3), e["joint_vel"].reshape(T, B, 4, 3), rho_fix)
    R = e["root_rot_mat"].reshape(T, B, 3, 3).transpose(0, 1, 3, 2)       # (row, col)
    q = e["root_quat"]
    yaw = np.arctan2(2.0 * (q[..., 0] * q[..., 3] + q[..., 1] * q[..., 2]),
                     1.0 - 2.0 * (q[..., 2] ** 2 + q[..., 3] ** 2))
    c, s, z, o = np.cos(yaw), np.sin(yaw), np.zeros_like(yaw), np.ones_like(yaw)
    rot_z = np.stack([c, s, z, -s, c, z, z, z, o], -1)                    # col-major
    foot_pos_abs = np.einsum("tbij,tblj->tbli", R, p).reshape(T, B, 12)
    root_lin_vel = rng.normal(0, 0.4, (T, B, 3))
    root_pos = np.cumsum(root_lin_vel * dt, 0) + np.array([0.0, 0.0, 0.28]) + rng.normal(0, 0.01, (1, B, 3))
    root_lin_vel_d = np.stack([rng.uniform(-0.6, 0.6, (T, B)), rng.uniform(-0.3, 0.3, (T, B)),
                               np.zeros((T, B))], -1)
    grf = np.stack([rng.normal(0, 15, (T, B, 4)), rng.normal(0, 15, (T, B, 4)),
                    rng.uniform(0, 120, (T, B, 4))], -1).reshape(T, B, 12)
    mode = np.broadcast_to(np.where(np.arange(B) % 4 == 3, 0, 1).astype(np.int32), (T, B)).copy()
    return dict(dt=np.full((T, B), dt), movement_mode=mode, root_pos=root_pos, root_lin_vel=root_lin_vel,
                root_lin_vel_d=root_lin_vel_d, root_rot_mat=e["root_rot_mat"], root_rot_mat_z=rot_z,
                foot_pos_abs=foot_pos_abs, foot_force=rng.uniform(-5, 60, (T, B, 4)),
                root_euler_d=rng.normal(0, 0.1, (T, B, 3)),
                j_foot=np.ascontiguousarray(J.transpose(0, 1, 2, 4, 3)).reshape(T, B, 36),
                foot_forces_grf=grf, joint_pos=e["joint_pos"], joint_vel=e["joint_vel"],
                root_quat=e["root_quat"], imu_acc=e["imu_acc"], imu_ang_vel=e["imu_ang_vel"])

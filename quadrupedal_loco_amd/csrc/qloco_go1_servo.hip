// qloco_go1_servo.hip -- one iteration of the go1 sim servo loop, batched
// (gfx950, fp64, no FMA contraction).
//
// Replaces servo.cpp:675-1330 (+ the go1_gait_data row of :1333-1433) of
// unitree_ros/go1_rt_control/src/servo_control for B robots started together:
//   go1_servo_kernel<false>  gait branch: Euler angles, Forward_kinematics_g and
//                            the measured foot velocity (:690-755), the
//                            /control2rtmpc/state row (:758-762), counters, the
//                            15 Butterworth filters, the per-mode targets and
//                            Inverse_kinematics_g (:889-1051), the force block's
//                            glue (:1052-1209, the operation order of
//                            servo_glue_kernel in qloco_servo.hip), the joint
//                            commands (:1265-1296) and the updates of :1318-1330
//   go1_servo_kernel<true>   stand-up branch (:769-809) in place of :889-1209
// then, in the gait branch and on the same stream, qloco_force_qp_solve_ordered
// and qloco_joint_torques (:1216-1243) on the arrays the kernel left in the
// workspace, and go1_gait_data_kernel when the row is asked for.
//
// Mapping: four lanes per robot, one leg per lane.  The per-leg work (FK with
// its Jacobian, up to 15 Newton steps of IK with a 3 x 3 inverse each) runs on
// every lane; the per-robot filters are spread over the quad (lane 0 com_des,
// 1 rfoot_des, 2 lfoot_des, 3 coma_des + thetaacc_des) and their outputs go
// round by DPP quad_perm broadcasts, no LDS.  The Euler angles, the body
// targets and the glue are computed by all four lanes from the same values
// (the same bits on each) and stored by the quad's first lane.  A robot per
// lane would hold four legs' FK / IK state live at once; this form needs one.
// The quad of a robot takes every quad-level branch together, so the
// broadcasts always see four active lanes; the IK loop diverges per lane and
// holds no cross-lane move.
//
// Memory: AoS fp64 rows per robot (3 per leg, 12 per robot), read and written
// by consecutive lanes.  The arrays the force QP and compute_joint_torques read
// are written once, by this kernel, in the layout those launches take.
#include <math.h>
#include <string.h>

#include "qloco_common.hpp"
#include "qloco_kin_core.hpp"

namespace qloco {
namespace go1servo {

constexpr double MASS = 12.0;  // gait::mass (go1_rt_control Robotpara :29)
constexpr double G = 9.8;      // gait::_g (:48)
// Momentum_sum, servo.cpp:375-377 (row-major)
__constant__ double c_momentum[9] = QLOCO_MOMENTUM_SUM;

constexpr int NF = QLOCO_GO1_SERVO_FILTERS;

struct Ws {  // byte offsets; doubles first, then int32
  int64_t coef, filt, angle, fhome, bhome, bpdes, brdes, fdes, rold, mold, compre, vrel, vest, ref[6],
      flr, fsum, fref, grf, tau, guess, rel, mea, jaco, count, tint, swing, rs, qps, st, ord, total;
};
__host__ __device__ inline Ws layout(int64_t B) {
  auto al = [](int64_t x) { return (x + 255) & ~(int64_t)255; };
  Ws w;
  int64_t o = 0;
  auto d = [&](int64_t per) { const int64_t at = o; o = al(o + 8 * per * B); return at; };
  auto i = [&](int64_t per) { const int64_t at = o; o = al(o + 4 * per * B); return at; };
  w.coef = o;
  o = al(o + 8 * 6 * NF);
  w.filt = d(5 * NF);
  w.angle = d(12);
  w.fhome = d(12);
  w.bhome = d(3);
  w.bpdes = d(3);
  w.brdes = d(3);
  w.fdes = d(12);
  w.rold = d(12);
  w.mold = d(12);
  w.compre = d(3);
  w.vrel = d(12);
  w.vest = d(12);
  for (int f = 0; f < 6; ++f) w.ref[f] = d(3);  // com_des, rfoot_des, lfoot_des, coma_des, thetaacc_des, comv_des
  w.flr = d(6);
  w.fsum = d(6);
  w.fref = d(12);
  w.grf = d(12);
  w.tau = d(12);
  w.guess = d(12);
  w.rel = d(12);
  w.mea = d(12);
  w.jaco = d(36);
  w.count = i(1);
  w.tint = i(1);
  w.swing = i(4);
  w.rs = i(1);
  w.qps = i(1);
  w.st = i(1);
  w.ord = o;  // the force QP's grouping workspace (qloco_force_order_ws_len)
  o = al(o + 4 * (2 * B + 2 * QLOCO_FORCE_CLASSES));
  w.total = o;
  return w;
}

template <int K>
__device__ __forceinline__ double quad_bcast(double v) {  // lane K of the caller's quad
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), K * 0x55, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), K * 0x55, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}

// Utils::quat_to_euler (utils/Utils.cpp:7-33), with its clamp of the asin argument
__device__ __forceinline__ void quat_euler(const double q[4], double e[3]) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double y_sqr = y * y;
  const double t0 = 2.0 * (w * x + y * z);
  const double t1 = 1.0 - 2.0 * (x * x + y_sqr);
  e[0] = atan2(t0, t1);
  double t2 = 2.0 * (w * y - z * x);
  t2 = t2 > 1.0 ? 1.0 : t2;
  t2 = t2 < -1.0 ? -1.0 : t2;
  e[1] = asin(t2);
  const double t3 = 2.0 * (w * z + x * y);
  const double t4 = 1.0 - 2.0 * (y_sqr + z * z);
  e[2] = atan2(t3, t4);
}

// butterworthLPF::filter (Filter/butterworthLPF.cpp:103-120) on the memory m[5]
// = y_p, y_pp, x_p, x_pp, i
__device__ __forceinline__ double butter(const double *__restrict__ c, double *__restrict__ m,
                                         double y) {
  const double y_p = m[0], y_pp = m[1], x_p = m[2], x_pp = m[3], i = m[4];
  double out;
  if (i > 2.0) {
    out = c[0] * y + c[1] * y_p + c[2] * y_pp + c[3] * x_p + c[4] * x_pp;
  } else {
    out = x_p + c[5] * (y - x_p);
    m[4] = i + 1.0;
  }
  m[1] = y_p;
  m[0] = y;
  m[3] = x_p;
  m[2] = out;
  return out;
}

struct TickArgs {
  int64_t B;
  char *ws;
  const double *q_mea, *quat, *gait, *y_off;
  const int32_t *mode;
  double *q_cmd, *ctrl;
  qloco_go1_servo_diag d;
  double target[12];
  double percent, dtx, t_walk_start, pitch_w, half_hip;
  int n_t_int, n_period, ros_gt1;
  // per-robot bodies (qloco_go1_servo_tick_body) or NULL, read by the gait
  // branch only: mass and momentum of F_sum.  A refused row takes the constants
  // as a stand-in, so nothing non-finite enters the workspace; the force QP
  // refuses the robot.
  const qloco_force_body *body;
};

template <bool HOMING>
__global__ __launch_bounds__(256) void go1_servo_kernel(const TickArgs a) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t r = gid >> 2;
  const int l = (int)(gid & 3);
  if (r >= a.B) return;  // whole quads leave together
  const Ws L = layout(a.B);
  const int64_t g3 = r * 12 + 3 * l;  // this leg's row of a [B*12] array
  auto D = [&](int64_t off) { return reinterpret_cast<double *>(a.ws + off); };
  auto I = [&](int64_t off) { return reinterpret_cast<int32_t *>(a.ws + off); };
  const kin::LegConst k = kin::leg_const(l);

  // ---- measured state (:690-755)
  const double qt[4] = {a.quat[4 * r], a.quat[4 * r + 1], a.quat[4 * r + 2], a.quat[4 * r + 3]};
  double e_est[3];
  quat_euler(qt, e_est);
  const double qm[3] = {a.q_mea[g3], a.q_mea[g3 + 1], a.q_mea[g3 + 2]};
  double mea[3], Jest[9];
  {
    double R[9];
    const double P0[3] = {0.0, 0.0, 0.0};  // body_p_est
    kin::body_rot(e_est, R);
    kin::fk(k, true, R, P0, qm, mea, Jest);
  }
  double vest[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    vest[c] = D(L.vest)[g3 + c];
    if (a.ros_gt1) vest[c] = (mea[c] - D(L.mold)[g3 + c]) / a.dtx;
    D(L.vest)[g3 + c] = vest[c];
    D(L.mea)[g3 + c] = mea[c];
  }
  // ---- /control2rtmpc/state (:758-762): state_feedback as the previous tick left it
  int count = I(L.count)[r];
  {
    const int t_prev = I(L.tint)[r];
    for (int j = l; j < QLOCO_CTRL_MSG_LEN; j += 4)
      a.ctrl[r * QLOCO_CTRL_MSG_LEN + j] = (j == 0) ? (double)t_prev : 0.0;
  }
  if (a.d.body_r_est && l == 0)
    for (int c = 0; c < 3; ++c) a.d.body_r_est[r * 3 + c] = e_est[c];
  if (a.d.foot_rel_mea)
    for (int c = 0; c < 3; ++c) a.d.foot_rel_mea[g3 + c] = mea[c];
  if (a.d.v_est_rel)
    for (int c = 0; c < 3; ++c) a.d.v_est_rel[g3 + c] = vest[c];
  if (a.d.Jaco_est)
    for (int c = 0; c < 9; ++c) a.d.Jaco_est[r * 36 + 9 * l + c] = Jest[c];

  double qd[3], fdes[3], rel[3], bp[3], br[3], com[3];
  auto REF = [&](int f, int c) -> double & { return D(L.ref[f])[r * 3 + c]; };
  int nup = 0;
  if (HOMING) {
    // ---- stand-up (:769-809)
    const double tg[3] = {
        l == 0 ? a.target[0] : l == 1 ? a.target[3] : l == 2 ? a.target[6] : a.target[9],
        l == 0 ? a.target[1] : l == 1 ? a.target[4] : l == 2 ? a.target[7] : a.target[10],
        l == 0 ? a.target[2] : l == 1 ? a.target[5] : l == 2 ? a.target[8] : a.target[11]};
#pragma unroll
    for (int c = 0; c < 3; ++c) qd[c] = qm[c] * (1.0 - a.percent) + tg[c] * a.percent;
    double J[9];
    kin::fk_local(k, qd, rel, J);  // FR_foot_des = FR_foot_relative_des = Forward_kinematics
    const double z = -(quad_bcast<0>(rel[2]) + quad_bcast<1>(rel[2]) + quad_bcast<2>(rel[2]) +
                       quad_bcast<3>(rel[2])) / 4.0;
    fdes[0] = rel[0];
    fdes[1] = rel[1];
    fdes[2] = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      bp[c] = D(L.bpdes)[r * 3 + c];
      br[c] = D(L.brdes)[r * 3 + c];
      com[c] = REF(0, c);
      D(L.fhome)[g3 + c] = fdes[c];
    }
    bp[2] = z;
    if (l == 0) {
      D(L.bhome)[r * 3 + 2] = z;
      D(L.bpdes)[r * 3 + 2] = z;
    }
  } else {
    // ---- counters (:891-893)
    count += 1;
    const int t_int = (int)round((double)(count / a.n_t_int));  // integer division, as written
    // ---- the 15 filters (:898-931), three per lane and thetaacc_des on lane 3
    const double *gm = a.gait + r * QLOCO_GAIT_MSG_LEN;
    const int slot = l == 0 ? 0 : l == 1 ? 9 : l == 2 ? 6 : 39;
    const double *cf = D(L.coef);
    double *fm = D(L.filt) + r * (5 * NF);
    double v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = butter(cf + 6 * (3 * l + c), fm + 5 * (3 * l + c), gm[slot + c]);
    double rf[3], lf[3], ca[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      com[c] = quad_bcast<0>(v[c]);
      rf[c] = quad_bcast<1>(v[c]);
      lf[c] = quad_bcast<2>(v[c]);
      ca[c] = quad_bcast<3>(v[c]);
    }
    if (l == 3) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double th = butter(cf + 6 * (12 + c), fm + 5 * (12 + c), gm[73 + c]);
        REF(4, c) = th;
        if (a.d.thetaacc_des) a.d.thetaacc_des[r * 3 + c] = th;
      }
    }
    double cv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      cv[c] = REF(5, c);
      if (count > 0) cv[c] = (com[c] - D(L.compre)[r * 3 + c]) / a.dtx;
      bp[c] = D(L.bpdes)[r * 3 + c];
      br[c] = D(L.brdes)[r * 3 + c];
      fdes[c] = D(L.fdes)[g3 + c];
    }
    const int mode = a.mode[r];
    const double yo = a.y_off[r];
    // ---- per-mode targets (:933-1033); theta_des = 0
    if ((double)count * a.dtx >= a.t_walk_start && (mode == 101 || mode == 102 || mode == 103)) {
      bp[0] = com[0];
      bp[1] = com[1] * yo;
      bp[2] = com[2];
      br[0] = 0.0;
      if (mode == 103) {
        const int dn = count - 3 * a.n_period;
        if (dn <= 0)
          br[0] = 0.0;  // body_r_des[0] = theta_des[1]
        else
          br[1] = -(0.1 * sin(a.pitch_w * (double)dn * a.dtx));
      } else {
        br[1] = 0.0;
      }
      br[2] = 0.0;
      // which of the two feet this leg follows: 101 right legs, 102 FR + RL, 103 fore legs
      const bool right = mode == 101 ? (l == 0 || l == 2) : mode == 102 ? (l == 0 || l == 3) : (l < 2);
      const double *hm = D(L.fhome) + g3;
      if (right) {
        fdes[0] = hm[0] + rf[0];
        fdes[1] = hm[1] + rf[1] + a.half_hip;
        fdes[2] = hm[2] + rf[2];
      } else {
        fdes[0] = hm[0] + lf[0];
        fdes[1] = hm[1] + lf[1] - a.half_hip;
        fdes[2] = hm[2] + lf[2];
      }
    }
    // ---- Inverse_kinematics_g from the previous angle_des (:1036-1051)
    double Jk[9];
    {
      double R[9], p[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) qd[c] = D(L.angle)[g3 + c];
      kin::body_rot(br, R);
      kin::fk(k, true, R, bp, qd, p, Jk);
      nup = kin::ik_newton(k, true, R, bp, fdes, qd, p, Jk);
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) D(L.jaco)[r * 36 + 9 * l + c] = Jk[c];
    if (a.d.Jaco)
      for (int c = 0; c < 9; ++c) a.d.Jaco[r * 36 + 9 * l + c] = Jk[c];
    // ---- the force block's glue (:1052-1209), servo_glue_kernel's operation order
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      rel[c] = fdes[c] - bp[c];
      if (count > 0) D(L.vrel)[g3 + c] = (rel[c] - D(L.rold)[g3 + c]) / a.dtx;
      D(L.rel)[g3 + c] = rel[c];
    }
    double F_sum[6];
    double mass = MASS, mom[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) mom[c] = c_momentum[c];
    if (a.body) {
      const double *row = reinterpret_cast<const double *>(a.body + r);
      if (force_body_ok(row)) {
        mass = row[0];
#pragma unroll
        for (int c = 0; c < 9; ++c) mom[c] = row[6 + c];
      }
    }
    F_sum[0] = mass * ca[0];
    F_sum[1] = mass * ca[1];
    F_sum[2] = mass * G + mass * ca[2];  // mass * G: MASS * G as the compiler folded it when mass = 12
#pragma unroll
    for (int i = 0; i < 3; ++i)
      F_sum[3 + i] = mom[3 * i + 0] * ca[0] + mom[3 * i + 1] * ca[1] + mom[3 * i + 2] * ca[2];
    const double v0 = lf[0] - rf[0], v1 = lf[1] - rf[1], v2 = lf[2] - rf[2];
    const double c0 = com[0] - rf[0], c1 = com[1] - rf[1], c2 = com[2] - rf[2];
    const double rlleg_dis = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
    const double com_rleg_dis = v0 * c0 + v1 * c1 + v2 * c2;
    const double raw = com_rleg_dis / rlleg_dis;
    const double raw1 = (1.0 < raw) ? 1.0 : raw;        // std::min(raw, 1.0)
    const double rleg_com = (raw1 < 0.0) ? 0.0 : raw1;  // std::max(raw1, 0.0)
    const int rs = (int)gm[99];                         // right_support = slow_mpc_gait(99) (:681)
    if (l == 0) {
      int32_t *sw = I(L.swing) + r * 4;
      double F[6];
      int s0 = sw[0], s1 = sw[1], s2 = sw[2], s3 = sw[3];
      if (rs == 0) {
        F[0] = F_sum[0]; F[1] = F_sum[1]; F[2] = F_sum[2]; F[3] = 0; F[4] = 0; F[5] = 0;
        if (mode == 101) { s0 = 1; s2 = 1; s1 = 0; s3 = 0; }
        else if (mode == 102) { s0 = 0; s3 = 0; s1 = 1; s2 = 1; }
        else if (mode == 103) { s0 = 1; s1 = 1; s2 = 0; s3 = 0; }
      } else if (rs == 1) {
        F[0] = 0; F[1] = 0; F[2] = 0; F[3] = F_sum[0]; F[4] = F_sum[1]; F[5] = F_sum[2];
        if (mode == 101) { s0 = 0; s2 = 0; s1 = 1; s3 = 1; }
        else if (mode == 102) { s0 = 1; s3 = 1; s1 = 0; s2 = 0; }
        else if (mode == 103) { s0 = 0; s1 = 0; s2 = 1; s3 = 1; }
      } else {
        F[0] = F_sum[0] * rleg_com; F[3] = F_sum[0] - F[0];
        F[1] = F_sum[1] * rleg_com; F[4] = F_sum[1] - F[1];
        F[2] = F_sum[2] * rleg_com; F[5] = F_sum[2] - F[2];
        s0 = s1 = s2 = s3 = 0;
      }
      sw[0] = s0; sw[1] = s1; sw[2] = s2; sw[3] = s3;
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        D(L.fsum)[r * 6 + c] = F_sum[c];
        D(L.flr)[r * 6 + c] = F[c];
      }
      I(L.rs)[r] = rs;
      I(L.count)[r] = count;
      I(L.tint)[r] = t_int;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        REF(0, c) = com[c];
        REF(1, c) = rf[c];
        REF(2, c) = lf[c];
        REF(3, c) = ca[c];
        REF(5, c) = cv[c];
        D(L.bpdes)[r * 3 + c] = bp[c];
        D(L.brdes)[r * 3 + c] = br[c];
      }
    }
  }
  // ---- joint commands (:776, :1265-1296) and the updates of :1318-1330
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    a.q_cmd[g3 + c] = qd[c];
    D(L.angle)[g3 + c] = qd[c];
    D(L.fdes)[g3 + c] = fdes[c];
    D(L.rold)[g3 + c] = rel[c];
    D(L.mold)[g3 + c] = mea[c];
  }
  if (l == 0)
    for (int c = 0; c < 3; ++c) D(L.compre)[r * 3 + c] = com[c];
  // ---- the members after the tick, for whoever asked
  if (a.d.angle_des)
    for (int c = 0; c < 3; ++c) a.d.angle_des[g3 + c] = qd[c];
  if (a.d.foot_des)
    for (int c = 0; c < 3; ++c) a.d.foot_des[g3 + c] = fdes[c];
  if (a.d.ik_updates) a.d.ik_updates[r * 4 + l] = nup;
  if (l == 0) {
    if (a.d.body_p_des)
      for (int c = 0; c < 3; ++c) a.d.body_p_des[r * 3 + c] = bp[c];
    if (a.d.body_r_des)
      for (int c = 0; c < 3; ++c) a.d.body_r_des[r * 3 + c] = br[c];
    double *const outs[6] = {a.d.com_des, a.d.rfoot_des, a.d.lfoot_des, a.d.coma_des,
                             HOMING ? a.d.thetaacc_des : nullptr, a.d.comv_des};
#pragma unroll
    for (int f = 0; f < 6; ++f)
      if (outs[f])
        for (int c = 0; c < 3; ++c) outs[f][r * 3 + c] = REF(f, c);
    if (a.d.F_sum)
      for (int c = 0; c < 6; ++c) a.d.F_sum[r * 6 + c] = D(L.fsum)[r * 6 + c];
    if (a.d.Force_L_R)
      for (int c = 0; c < 6; ++c) a.d.Force_L_R[r * 6 + c] = D(L.flr)[r * 6 + c];
    if (a.d.swing)
      for (int c = 0; c < 4; ++c) a.d.swing[r * 4 + c] = I(L.swing)[r * 4 + c];
  }
  if (HOMING && a.d.Jaco)
    for (int c = 0; c < 9; ++c) a.d.Jaco[r * 36 + 9 * l + c] = D(L.jaco)[r * 36 + 9 * l + c];
}

// joint2simulation (:1335-1433), one entry per lane
__global__ __launch_bounds__(256) void go1_gait_data_kernel(int64_t B, const char *ws,
                                                            const double *__restrict__ q_cmd,
                                                            const double *__restrict__ q_mea,
                                                            double *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * QLOCO_GO1_GAIT_DATA_LEN) return;
  const int64_t r = i / QLOCO_GO1_GAIT_DATA_LEN;
  const int j = (int)(i - r * QLOCO_GO1_GAIT_DATA_LEN);
  const Ws L = layout(B);
  auto D = [&](int64_t off) { return reinterpret_cast<const double *>(ws + off); };
  double v = 0.0;
  if (j < 12) v = q_cmd[r * 12 + j];
  else if (j < 24) v = q_mea[r * 12 + j - 12];
  else if (j < 36) v = D(L.fdes)[r * 12 + j - 24];
  else if (j < 48) v = D(L.mea)[r * 12 + j - 36] + D(L.bpdes)[r * 3 + (j - 36) % 3];
  else if (j < 51) v = D(L.bpdes)[r * 3 + j - 48];
  else if (j < 54) v = D(L.brdes)[r * 3 + j - 51];
  else if (j < 60) v = D(L.flr)[r * 6 + j - 54];
  else if (j < 66) v = 0.0;
  else if (j < 78) v = D(L.fref)[r * 12 + j - 66];
  else if (j < 90) v = D(L.tau)[r * 12 + j - 78];
  out[i] = v;
}

// where entry j of a robot's dense record lives: a double (p) or an int32 (q)
__device__ __forceinline__ void locate(const Ws &L, char *ws, int64_t r, int j, double **p,
                                       int32_t **q) {
  *p = nullptr;
  *q = nullptr;
  auto D = [&](int64_t off, int per, int at) {
    *p = reinterpret_cast<double *>(ws + off) + r * per + at;
  };
  auto I = [&](int64_t off, int per, int at) {
    *q = reinterpret_cast<int32_t *>(ws + off) + r * per + at;
  };
  if (j < 75) D(L.filt, 75, j);
  else if (j < 87) D(L.angle, 12, j - 75);
  else if (j < 99) D(L.fhome, 12, j - 87);
  else if (j < 102) D(L.bhome, 3, j - 99);
  else if (j < 105) D(L.bpdes, 3, j - 102);
  else if (j < 108) D(L.brdes, 3, j - 105);
  else if (j < 120) D(L.fdes, 12, j - 108);
  else if (j < 132) D(L.rold, 12, j - 120);
  else if (j < 144) D(L.mold, 12, j - 132);
  else if (j < 147) D(L.compre, 3, j - 144);
  else if (j < 159) D(L.vrel, 12, j - 147);
  else if (j < 171) D(L.vest, 12, j - 159);
  else if (j < 172) I(L.count, 1, 0);
  else if (j < 176) I(L.swing, 4, j - 172);
  else if (j < 188) D(L.fref, 12, j - 176);
  else if (j < 200) D(L.grf, 12, j - 188);
  else if (j < 212) D(L.tau, 12, j - 200);
  else if (j < 230)  // six [B*3] arrays one after the other, equally spaced
    D(L.ref[0] + ((j - 212) / 3) * (L.ref[1] - L.ref[0]), 3, (j - 212) % 3);
  else if (j < 231) I(L.tint, 1, 0);
  else if (j < 237) D(L.flr, 6, j - 231);
  else if (j < 243) D(L.fsum, 6, j - 237);
  else if (j < 279) D(L.jaco, 36, j - 243);
  else if (j < 280) I(L.qps, 1, 0);
  else if (j < 281) I(L.st, 1, 0);
}

template <bool SET>
__global__ __launch_bounds__(256) void go1_state_kernel(int64_t B, char *ws, double *state) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * QLOCO_GO1_SERVO_STATE) return;
  const int64_t r = i / QLOCO_GO1_SERVO_STATE;
  const int j = (int)(i - r * QLOCO_GO1_SERVO_STATE);
  const Ws L = layout(B);
  double *p;
  int32_t *q;
  locate(L, ws, r, j, &p, &q);
  if (SET) {
    if (p) *p = state[i];
    if (q) *q = (int32_t)state[i];
  } else {
    state[i] = p ? *p : q ? (double)*q : 0.0;
  }
}

struct InitArgs {
  int64_t B;
  char *ws;
  double z_c, half_hip;
  qloco_butter_coef filter[NF];
};

// paramInit (:300-470) and main's member setup (:556-616): everything 0 but
// com_des(2) = Z_c and the feet's y = -+ HALF_HIP_WIDTH (:450-453)
__global__ __launch_bounds__(256) void go1_init_kernel(const InitArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const Ws L = layout(a.B);
  const int64_t n = L.total / 4;
  if (i >= n) return;
  reinterpret_cast<int32_t *>(a.ws)[i] = 0;
}
__global__ __launch_bounds__(256) void go1_init2_kernel(const InitArgs a) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const Ws L = layout(a.B);
  if (r < NF) {
    double *c = reinterpret_cast<double *>(a.ws + L.coef) + 6 * r;
    // a static walk over the kernel argument: no dynamic index into it
#pragma unroll
    for (int f = 0; f < NF; ++f)
      if (f == r) {
        c[0] = a.filter[f].b0;
        c[1] = a.filter[f].b1;
        c[2] = a.filter[f].b2;
        c[3] = a.filter[f].a1;
        c[4] = a.filter[f].a2;
        c[5] = a.filter[f].a;
      }
  }
  if (r >= a.B) return;
  reinterpret_cast<double *>(a.ws + L.ref[0])[r * 3 + 2] = a.z_c;
  reinterpret_cast<double *>(a.ws + L.ref[1])[r * 3 + 1] = -a.half_hip;
  reinterpret_cast<double *>(a.ws + L.ref[2])[r * 3 + 1] = a.half_hip;
}

bool params_ok(const qloco_go1_servo_params *p) {
  return p && p->rt_frequency > 0.0 && p->stand_duration > 0.0 && p->dtx > 0.0 &&
         p->dt_mpc_slow > 0.0 && p->t_period > 0.0 && round(p->dt_mpc_slow / p->dtx) >= 1.0 &&
         round(p->dt_mpc_slow / p->dtx) < 1e9 && round(p->t_period / p->dtx) < 1e8;
}

}  // namespace go1servo
}  // namespace qloco

using namespace qloco;

static void butter_coef_init(double f_sample, double f_cutoff, qloco_butter_coef *c) {
  // butterworthLPF::init (Filter/butterworthLPF.cpp:83-99), its expressions and its pi
  const double ff = f_cutoff / f_sample;
  const double ita = 1.0 / tan(3.14159265359 * ff);
  const double q = sqrt(2.0);
  c->b0 = 1.0 / (1.0 + q * ita + ita * ita);
  c->b1 = 2 * c->b0;
  c->b2 = c->b0;
  c->a1 = 2.0 * (ita * ita - 1.0) * c->b0;
  c->a2 = -(1.0 - q * ita + ita * ita) * c->b0;
  c->a = (2.0 * 3.14159265359 * ff) / (2.0 * 3.14159265359 * ff + 1.0);
}

extern "C" void qloco_go1_servo_params_default(qloco_go1_servo_params *p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->rt_frequency = 1000;
  p->stand_duration = 5;
  p->dtx = 0.005;
  p->dt_mpc_slow = 0.025;
  p->t_period = 0.7;
  p->t_walk_start = 0.6;
  p->pi = 3.141526;
  p->half_hip_width = 0.12675;
  p->z_c = 0.309458;
  const double target[12] = {0, 0.87, -1.5, 0, 0.87, -1.5, 0, 0.87, -1.5, 0, 0.87, -1.5};
  memcpy(p->target_pos, target, sizeof(target));
  // servo.cpp:579-599: LPF1-11 at 3 Hz, LPF12-18 at 10 Hz; live here are LPF1-3, 7-18
  const double fs = 1 / p->dtx;
  for (int f = 0; f < go1servo::NF; ++f) butter_coef_init(fs, f < 8 ? 3 : 10, &p->filter[f]);
  qloco_force_params_default(&p->force);
}

extern "C" int64_t qloco_go1_servo_workspace_bytes(int64_t batch) {
  if (batch <= 0) return -1;
  return go1servo::layout(batch).total;
}

extern "C" int qloco_go1_servo_init(const qloco_go1_servo_params *prm, int64_t batch,
                                    void *workspace, void *stream) {
  if (!go1servo::params_ok(prm) || batch <= 0 || batch > (INT32_MAX >> 2) || !workspace)
    return QLOCO_ERR_ARG;
  go1servo::InitArgs a;
  a.B = batch;
  a.ws = (char *)workspace;
  a.z_c = prm->z_c;
  a.half_hip = prm->half_hip_width;
  memcpy(a.filter, prm->filter, sizeof(a.filter));
  const int64_t n = go1servo::layout(batch).total / 4;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(go1servo::go1_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
  QLOCO_HIP_CHECK(hipGetLastError(), "go1_init_kernel launch");
  const int64_t m = batch > go1servo::NF ? batch : go1servo::NF;
  hipLaunchKernelGGL(go1servo::go1_init2_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, a);
  QLOCO_HIP_CHECK(hipGetLastError(), "go1_init2_kernel launch");
  return QLOCO_OK;
}

extern "C" int qloco_go1_servo_tick_body(const qloco_go1_servo_params *prm, int64_t batch,
                                         void *workspace, int64_t n_count, const double *q_mea,
                                         const double *quat, const double *gait_msg,
                                         const int32_t *gait_mode, const double *y_offset,
                                         double *q_cmd, double *ctrl_msg, double *tau,
                                         double *grf_opt, const qloco_go1_servo_diag *diag,
                                         double *gait_data, const qloco_force_body *body,
                                         void *stream) {
  if (!go1servo::params_ok(prm) || batch <= 0 || batch > (INT32_MAX >> 2) || n_count < 0 ||
      n_count >= INT32_MAX || !workspace || !q_mea || !quat || !gait_msg || !gait_mode ||
      !y_offset || !q_cmd || !ctrl_msg || !tau || !grf_opt)
    return QLOCO_ERR_ARG;
  const go1servo::Ws L = go1servo::layout(batch);
  char *w = (char *)workspace;
  const hipStream_t st = (hipStream_t)stream;
  go1servo::TickArgs a;
  memset(&a, 0, sizeof(a));
  a.B = batch;
  a.ws = w;
  a.q_mea = q_mea;
  a.quat = quat;
  a.gait = gait_msg;
  a.y_off = y_offset;
  a.mode = gait_mode;
  a.q_cmd = q_cmd;
  a.ctrl = ctrl_msg;
  if (diag) a.d = *diag;
  memcpy(a.target, prm->target_pos, sizeof(a.target));
  a.dtx = prm->dtx;
  a.t_walk_start = prm->t_walk_start;
  a.pitch_w = 2 * prm->pi / (2 * prm->t_period);  // pitch_angle_W (:998)
  a.half_hip = prm->half_hip_width;
  a.n_t_int = (int)round(prm->dt_mpc_slow / prm->dtx);  // :568
  a.n_period = (int)round(prm->t_period / prm->dtx);    // :616
  a.ros_gt1 = n_count + 1 > 1;                          // count_in_rt_ros (:675, :749)
  const double time_programming = 1.0 / prm->rt_frequency;  // :634
  const double t = (double)(int)n_count * time_programming;
  const bool homing = t <= prm->stand_duration;  // :769
  const double frac = t / prm->stand_duration;
  a.percent = frac * frac;  // pow(v, 2): the exactly rounded square
  a.body = homing ? nullptr : body;
  const dim3 grid((unsigned)((4 * batch + 255) / 256)), block(256);
  if (homing) {
    hipLaunchKernelGGL(go1servo::go1_servo_kernel<true>, grid, block, 0, st, a);
    QLOCO_HIP_CHECK(hipGetLastError(), "go1_servo_kernel (stand-up) launch");
  } else {
    hipLaunchKernelGGL(go1servo::go1_servo_kernel<false>, grid, block, 0, st, a);
    QLOCO_HIP_CHECK(hipGetLastError(), "go1_servo_kernel launch");
    // Dynam.force_distribution(body_p_des, leg_position, Force_L_R, gait_mode, y_offset,
    // rfoot_des, lfoot_des); Dynam.force_opt(body_p_des, FR..RL_foot_des, F_sum, gait_mode,
    // right_support, y_offset)  (:1216-1228)
    const double *bp = (const double *)(w + L.bpdes), *fd = (const double *)(w + L.fdes);
    const double *rf = (const double *)(w + L.ref[1]), *lf = (const double *)(w + L.ref[2]);
    double *fref = (double *)(w + L.fref);
    int rc = qloco_force_qp_solve_body(
        &prm->force, batch, bp, fd, (const double *)(w + L.flr), rf, lf, bp, fd,
        (const double *)(w + L.fsum), gait_mode, (const int32_t *)(w + L.rs), y_offset, fref,
        (double *)(w + L.grf), (double *)(w + L.guess), (int32_t *)(w + L.qps),
        (int32_t *)(w + L.st), nullptr, (int32_t *)(w + L.ord), body, stream);
    if (rc != QLOCO_OK) return rc;
    // compute_joint_torques for FR, FL, RR, RL (:1232-1248)
    rc = qloco_joint_torques(batch, (const double *)(w + L.jaco), (const int32_t *)(w + L.swing),
                             (const double *)(w + L.rel), (const double *)(w + L.mea),
                             (const double *)(w + L.vrel), (const double *)(w + L.vest), fref,
                             (double *)(w + L.tau), stream);
    if (rc != QLOCO_OK) return rc;
  }
  QLOCO_HIP_CHECK(hipMemcpyAsync(tau, w + L.tau, sizeof(double) * 12 * batch,
                                 hipMemcpyDeviceToDevice, st),
                  "Legs_torque copy");
  QLOCO_HIP_CHECK(hipMemcpyAsync(grf_opt, w + L.grf, sizeof(double) * 12 * batch,
                                 hipMemcpyDeviceToDevice, st),
                  "grf_opt copy");
  // a refused robot's workspace rows are finite (they did not move); what the caller sees is NaN
  if (a.body) {
    const int rc = force_body_mark_refused(batch, body, tau, grf_opt, st);
    if (rc != QLOCO_OK) return rc;
  }
  if (diag && diag->qp_solution)
    QLOCO_HIP_CHECK(hipMemcpyAsync(diag->qp_solution, w + L.qps, sizeof(int32_t) * batch,
                                   hipMemcpyDeviceToDevice, st),
                    "qp_solution copy");
  if (diag && diag->status)
    QLOCO_HIP_CHECK(hipMemcpyAsync(diag->status, w + L.st, sizeof(int32_t) * batch,
                                   hipMemcpyDeviceToDevice, st),
                    "status copy");
  if (gait_data) {
    const int64_t n = batch * QLOCO_GO1_GAIT_DATA_LEN;
    hipLaunchKernelGGL(go1servo::go1_gait_data_kernel, dim3((unsigned)((n + 255) / 256)),
                       dim3(256), 0, st, batch, (const char *)w, (const double *)q_cmd, q_mea,
                       gait_data);
    QLOCO_HIP_CHECK(hipGetLastError(), "go1_gait_data_kernel launch");
  }
  return QLOCO_OK;
}

extern "C" int qloco_go1_servo_tick(const qloco_go1_servo_params *prm, int64_t batch,
                                    void *workspace, int64_t n_count, const double *q_mea,
                                    const double *quat, const double *gait_msg,
                                    const int32_t *gait_mode, const double *y_offset,
                                    double *q_cmd, double *ctrl_msg, double *tau, double *grf_opt,
                                    const qloco_go1_servo_diag *diag, double *gait_data,
                                    void *stream) {
  return qloco_go1_servo_tick_body(prm, batch, workspace, n_count, q_mea, quat, gait_msg, gait_mode,
                                   y_offset, q_cmd, ctrl_msg, tau, grf_opt, diag, gait_data, nullptr,
                                   stream);
}

extern "C" int qloco_go1_servo_get_state(int64_t batch, const void *workspace, double *state,
                                         void *stream) {
  if (batch <= 0 || batch > (INT32_MAX >> 2) || !workspace || !state) return QLOCO_ERR_ARG;
  const int64_t n = batch * QLOCO_GO1_SERVO_STATE;
  hipLaunchKernelGGL(go1servo::go1_state_kernel<false>, dim3((unsigned)((n + 255) / 256)),
                     dim3(256), 0, (hipStream_t)stream, batch, (char *)workspace, state);
  QLOCO_HIP_CHECK(hipGetLastError(), "go1_state_kernel (get) launch");
  return QLOCO_OK;
}

extern "C" int qloco_go1_servo_set_state(int64_t batch, void *workspace, const double *state,
                                         void *stream) {
  if (batch <= 0 || batch > (INT32_MAX >> 2) || !workspace || !state) return QLOCO_ERR_ARG;
  const int64_t n = batch * QLOCO_GO1_SERVO_STATE;
  hipLaunchKernelGGL(go1servo::go1_state_kernel<true>, dim3((unsigned)((n + 255) / 256)),
                     dim3(256), 0, (hipStream_t)stream, batch, (char *)workspace,
                     (double *)state);
  QLOCO_HIP_CHECK(hipGetLastError(), "go1_state_kernel (set) launch");
  return QLOCO_OK;
}

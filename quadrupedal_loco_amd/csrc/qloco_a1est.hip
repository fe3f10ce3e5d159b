// qloco_a1est.hip -- batched A1 state estimation front end, fp64 like the
// reference (include/qloco.h sections 11 and 12).
//
// 11. A1 leg kinematics: the per-leg block of GazeboA1ROS::gt_pose_callback
//     (unitree_ros/a1_cpp_open_source/src/GazeboA1ROS.cpp:306-331):
//     A1Kinematics::fk / jac (legKinematics/A1Kinematics.cpp:39-130, the
//     generated closed forms, same expression order), foot_vel_rel = J qdot,
//     Quaternion::toRotationMatrix, Utils::quat_to_euler (Utils.cpp:7-33),
//     the yaw-only AngleAxis matrix and the body / world frame copies.
//     One leg per lane, legs FL, FR, RL, RR; consecutive lanes read and write
//     consecutive 3-vectors, so a wave touches one contiguous span per array.
//
// 12. A1BasicEKF (A1BasicEKF.cpp:7-164): init_state and update_estimation.
//     One robot per 32-lane group, two robots per one-wave workgroup.  C is a
//     selection / difference matrix (ctor :11-17), so C Pbar and C Pbar C' are
//     gathers of Pbar entries.  S = L L' (Cholesky-Crout, lane r keeps row r
//     in registers and publishes it to LDS column by column), then one
//     19-column forward substitution W = L^-1 [C Pbar | y - C xbar] with one
//     column per lane (L is read as LDS broadcasts), P = Pbar - W'W,
//     x = xbar + W'(L^-1 e).  The reference solves with fullPivHouseholderQr
//     twice; the two agree to rounding (tests/a1_est_ref.py).
//     Every loop has a fixed trip count; NaN inputs only propagate.
//
//     Workspace: QLOCO_A1_EKF_WS doubles per robot = x(18) | P packed lower
//     triangle, row by row (171) | pad to a 128-byte multiple.
//     LDS per robot: one 28x19 block (first the dense prior P, then L
//     packed, last W) | Pbar 18x18 | vectors = 7.7 KB.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "qloco.h"
#include "qloco_common.hpp"

namespace qloco {
namespace {

// ------------------------------------------------------------------ kinematics
// A1Kinematics::autoFunc_fk_derive (A1Kinematics.cpp:39-74): q, rho_opt, rho_fix
__device__ __forceinline__ void a1_fk(const double q[3], const double ro[3], const double rf[5],
                                      double p[3]) {
  const double t2 = cos(q[0]), t3 = cos(q[1]), t4 = cos(q[2]);
  const double t5 = sin(q[0]), t6 = sin(q[1]), t7 = sin(q[2]);
  double t8 = q[1] + q[2];
  double t9 = sin(t8);
  p[0] = (((rf[0] + ro[2] * t9) - rf[4] * t9) - t6 * rf[3]) + ro[0] * cos(t8);
  p[1] = ((((((((rf[1] + ro[1] * t2) + rf[2] * t2) + t3 * t5 * rf[3]) + ro[0] * t3 * t5 * t7) +
             ro[0] * t4 * t5 * t6) -
            ro[2] * t3 * t4 * t5) +
           ro[2] * t5 * t6 * t7) +
          rf[4] * t3 * t4 * t5) -
         rf[4] * t5 * t6 * t7;
  t8 = ro[0] * t2;
  t9 = ro[2] * t2;
  const double pt = rf[4] * t2;
  p[2] = (((((((ro[1] * t5 + rf[2] * t5) - t2 * t3 * rf[3]) - t8 * t3 * t7) - t8 * t4 * t6) +
            t9 * t3 * t4) -
           t9 * t6 * t7) -
          pt * t3 * t4) +
         pt * t6 * t7;
}

// A1Kinematics::autoFunc_d_fk_dq (A1Kinematics.cpp:76-130), column-major 3x3
__device__ __forceinline__ void a1_jac(const double q[3], const double ro[3], const double rf[5],
                                       double J[9]) {
  const double t2 = cos(q[0]), t3 = cos(q[1]), t4 = cos(q[2]);
  const double t5 = sin(q[0]), t6 = sin(q[1]), t7 = sin(q[2]);
  double t8 = q[1] + q[2];
  const double t9 = cos(t8);
  t8 = sin(t8);
  const double t12 = ro[0] * t9, t16 = ro[2] * t8, t17 = rf[4] * t8;
  const double t22 = (t12 + t16) + -t17;
  J[0] = 0.0;
  double a = ro[0] * t2;
  double b = ro[2] * t2;
  const double c = rf[4] * t2;
  J[1] = (((((((-ro[1] * t5 - rf[2] * t5) + t2 * t3 * rf[3]) + a * t3 * t7) + a * t4 * t6) -
            b * t3 * t4) +
           b * t6 * t7) +
          c * t3 * t4) -
         c * t6 * t7;
  J[2] = (((((((ro[1] * t2 + rf[2] * t2) + t3 * t5 * rf[3]) + ro[0] * t3 * t5 * t7) +
             ro[0] * t4 * t5 * t6) -
            ro[2] * t3 * t4 * t5) +
           ro[2] * t5 * t6 * t7) +
          rf[4] * t3 * t4 * t5) -
         rf[4] * t5 * t6 * t7;
  a = (ro[2] * t9 + -(rf[4] * t9)) + -(ro[0] * t8);
  J[3] = a - t3 * rf[3];
  b = ((t6 * rf[3] - t12) - t16) + t17;
  J[4] = -t5 * b;
  J[5] = t2 * b;
  J[6] = a;
  J[7] = t5 * t22;
  J[8] = -t2 * t22;
}

// Eigen Quaternion::toRotationMatrix, q = (w, x, y, z); column-major result
__device__ __forceinline__ void quat_rot(const double q[4], double R[9]) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1.0 - (tyy + tzz);
  R[3] = txy - twz;
  R[6] = txz + twy;
  R[1] = txy + twz;
  R[4] = 1.0 - (txx + tzz);
  R[7] = tyz - twx;
  R[2] = txz - twy;
  R[5] = tyz + twx;
  R[8] = 1.0 - (txx + tyy);
}

// Utils::quat_to_euler (Utils.cpp:7-33), with its clamp of the asin argument
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

struct KinArgs {
  qloco_a1_kin_params prm;
  int64_t n;  // legs = 4 * batch
  const double *joint_pos, *joint_vel, *root_quat, *root_pos, *root_lin_vel;
  double *foot_pos_rel, *j_foot, *foot_vel_rel, *root_rot_mat, *root_euler, *root_rot_mat_z;
  double *foot_pos_abs, *foot_vel_abs, *foot_pos_world, *foot_vel_world;
};

__device__ __forceinline__ void rot_apply(const double R[9], const double v[3], double o[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) o[k] = R[k] * v[0] + R[3 + k] * v[1] + R[6 + k] * v[2];
}

__global__ __launch_bounds__(256) void a1_leg_kin_kernel(KinArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const int64_t b = i >> 2;
  const int leg = (int)(i & 3);
  double rf[5], ro[3];
#pragma unroll
  for (int k = 0; k < 5; ++k) rf[k] = a.prm.rho_fix[leg][k];
#pragma unroll
  for (int k = 0; k < 3; ++k) ro[k] = a.prm.rho_opt[leg][k];
  const double q[3] = {a.joint_pos[3 * i], a.joint_pos[3 * i + 1], a.joint_pos[3 * i + 2]};
  const double qd[3] = {a.joint_vel[3 * i], a.joint_vel[3 * i + 1], a.joint_vel[3 * i + 2]};
  const double qt[4] = {a.root_quat[4 * b], a.root_quat[4 * b + 1], a.root_quat[4 * b + 2],
                        a.root_quat[4 * b + 3]};
  double p[3], J[9], v[3], R[9];
  a1_fk(q, ro, rf, p);
  a1_jac(q, ro, rf, J);
  rot_apply(J, qd, v);  // foot_vel_rel = J qdot (:322-324)
  quat_rot(qt, R);
#pragma unroll
  for (int k = 0; k < 3; ++k) a.foot_pos_rel[3 * i + k] = p[k];
  if (a.j_foot) {
#pragma unroll
    for (int k = 0; k < 9; ++k) a.j_foot[9 * i + k] = J[k];
  }
  if (a.foot_vel_rel) {
#pragma unroll
    for (int k = 0; k < 3; ++k) a.foot_vel_rel[3 * i + k] = v[k];
  }
  double pa[3], va[3];
  rot_apply(R, p, pa);
  rot_apply(R, v, va);
  if (a.foot_pos_abs) {
#pragma unroll
    for (int k = 0; k < 3; ++k) a.foot_pos_abs[3 * i + k] = pa[k];
  }
  if (a.foot_vel_abs) {
#pragma unroll
    for (int k = 0; k < 3; ++k) a.foot_vel_abs[3 * i + k] = va[k];
  }
  if (a.foot_pos_world) {
#pragma unroll
    for (int k = 0; k < 3; ++k) a.foot_pos_world[3 * i + k] = pa[k] + a.root_pos[3 * b + k];
  }
  if (a.foot_vel_world) {
#pragma unroll
    for (int k = 0; k < 3; ++k) a.foot_vel_world[3 * i + k] = va[k] + a.root_lin_vel[3 * b + k];
  }
  if (leg == 0) {
    if (a.root_rot_mat) {
#pragma unroll
      for (int k = 0; k < 9; ++k) a.root_rot_mat[9 * b + k] = R[k];
    }
    if (a.root_euler || a.root_rot_mat_z) {
      double e[3];
      quat_euler(qt, e);
      if (a.root_euler) {
#pragma unroll
        for (int k = 0; k < 3; ++k) a.root_euler[3 * b + k] = e[k];
      }
      if (a.root_rot_mat_z) {  // AngleAxisd(yaw, UnitZ).toRotationMatrix()
        const double c = cos(e[2]), s = sin(e[2]);
        double *z = a.root_rot_mat_z + 9 * b;
        z[0] = c;
        z[1] = s;
        z[2] = 0.0;
        z[3] = -s;
        z[4] = c;
        z[5] = 0.0;
        z[6] = 0.0;
        z[7] = 0.0;
        z[8] = (1.0 - c) + c;
      }
    }
  }
}

// ------------------------------------------------------------------------ EKF
constexpr int NX = 18;                  // STATE_SIZE
constexpr int NY = 28;                  // MEAS_SIZE
constexpr int NPK = NX * (NX + 1) / 2;  // packed P
constexpr int WSD = QLOCO_A1_EKF_WS;    // workspace doubles per robot
constexpr int GW = 32;                  // lanes per robot
constexpr int RPB = 2;                  // robots per (one-wave) workgroup
constexpr int NW = NX + 1;              // columns of W
// LDS map of one robot (doubles)
constexpr int L_OFF = 0;                      // dense prior P | L packed 406 | W 28x19
constexpr int PB_OFF = NY * NW;               // Pbar 18x18, then the posterior P
constexpr int V_OFF = PB_OFF + NX * NX;       // vectors
constexpr int V_IN = 0;                       // R 9 | acc 3 | omega 3 | fk 12 | fvel 12 | force 4
constexpr int V_X = 43, V_XBAR = 61, V_E = 79;
constexpr int LDS_ROBOT = V_OFF + 108;
static_assert(NY * (NY + 1) / 2 <= PB_OFF && NX * NX <= PB_OFF, "L and the prior P fit under W");
static_assert(WSD >= NX + NPK, "workspace record");

// the plus / minus column of row r of C (A1BasicEKF.cpp:11-17); -1: none
__host__ __device__ constexpr int c_plus(int r) {
  return r < 12 ? 6 + r : (r < 24 ? 3 + (r - 12) % 3 : 8 + 3 * (r - 24));
}
__host__ __device__ constexpr int c_minus(int r) { return r < 12 ? r % 3 : -1; }

// packed lower-triangle index t -> (i, j), j <= i
__device__ __forceinline__ void tri_decode(int t, int &i, int &j) {
  int r = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
  r += ((r + 1) * (r + 2) / 2 <= t) ? 1 : 0;
  r -= (r * (r + 1) / 2 > t) ? 1 : 0;
  i = r;
  j = t - r * (r + 1) / 2;
}

// The row loops below are unrolled in full (register rows); without a fence
// the scheduler hoists every LDS load of the later rows above the first row's
// arithmetic and runs out of registers.
__device__ __forceinline__ void sched_fence() { __builtin_amdgcn_sched_barrier(0); }

struct EkfArgs {
  qloco_a1_ekf_params prm;
  int64_t batch;
  double *ws;
  const double *dt;
  const int32_t *mode;
  const double *rot, *acc, *omega, *fk, *fvel, *force;
  double *root_pos, *root_lin_vel;
  uint8_t *contacts;
};

__global__ __launch_bounds__(64) void a1_ekf_update_kernel(EkfArgs a) {
  __shared__ double lds[RPB * LDS_ROBOT];
  const int lane = threadIdx.x & (GW - 1);
  const int grp = threadIdx.x / GW;
  int64_t rb = (int64_t)blockIdx.x * RPB + grp;
  const bool active = rb < a.batch;
  rb = active ? rb : a.batch - 1;  // the ragged tail recomputes the last robot, stores nothing
  double *sh = lds + grp * LDS_ROBOT;
  double *Lp = sh + L_OFF, *Pb = sh + PB_OFF, *vin = sh + V_OFF + V_IN, *xs = sh + V_OFF + V_X,
         *xbs = sh + V_OFF + V_XBAR, *es = sh + V_OFF + V_E;
  double *wsr = a.ws + rb * WSD;

  // 1. stage the inputs, x and the dense prior P (coalesced)
  for (int t = lane; t < 43; t += GW) {
    double v;
    if (t < 9) v = a.rot[rb * 9 + t];
    else if (t < 12) v = a.acc[rb * 3 + (t - 9)];
    else if (t < 15) v = a.omega[rb * 3 + (t - 12)];
    else if (t < 27) v = a.fk[rb * 12 + (t - 15)];
    else if (t < 39) v = a.fvel[rb * 12 + (t - 27)];
    else v = a.force[rb * 4 + (t - 39)];
    vin[t] = v;
  }
  if (lane < NX) xs[lane] = wsr[lane];
  for (int t = lane; t < NPK; t += GW) {
    int i, j;
    tri_decode(t, i, j);
    const double v = wsr[NX + t];
    Lp[i * NX + j] = v;
    Lp[j * NX + i] = v;
  }
  const double dt = a.dt[rb];
  const int mode = a.mode[rb];
  __syncthreads();

  // 2. contacts, u, xbar, Pbar = A P A' + Q, e = y - C xbar (:76-128)
  const double *Rm = vin, *acc = vin + 9, *om = vin + 12, *fk = vin + 15, *fv = vin + 27;
  double c[4], nz[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double t = vin[39 + i] / (100.0 - 0.0);
    const double m = (t < 0.0) ? 0.0 : t;         // std::max(t, 0.0)
    const double cw = (1.0 < m) ? 1.0 : m;        // std::min(m, 1.0)
    c[i] = (mode == 0) ? 1.0 : cw;
    nz[i] = 1.0 + (1.0 - c[i]) * 1e3;
  }
  double u[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) u[k] = Rm[k] * acc[0] + Rm[3 + k] * acc[1] + Rm[6 + k] * acc[2];
  u[2] = u[2] + -9.81;
  auto xbar_of = [&](int k) -> double {
    if (k < 3) return xs[k] + dt * xs[k + 3];
    if (k < 6) return xs[k] + dt * (k == 3 ? u[0] : (k == 4 ? u[1] : u[2]));
    return xs[k];
  };
  if (lane < NX) xbs[lane] = xbar_of(lane);
  for (int t = lane; t < NX * NX; t += GW) {
    const int i = t / NX, j = t - i * NX;
    const int i3 = i < 3 ? i + 3 : i, j3 = j < 3 ? j + 3 : j;
    // (A P)[i][.] = P[i][.] + dt P[i+3][.] (i < 3); then the same on columns
    const double apij = (i < 3) ? Lp[i * NX + j] + dt * Lp[i3 * NX + j] : Lp[i * NX + j];
    double v = apij;
    if (j < 3) {
      const double apij3 = (i < 3) ? Lp[i * NX + j3] + dt * Lp[i3 * NX + j3] : Lp[i * NX + j3];
      v = apij + apij3 * dt;
    }
    if (i == j) {
      double qd;
      if (i < 3) qd = a.prm.process_noise_pimu * dt / 20.0;
      else if (i < 6) qd = a.prm.process_noise_vimu * dt * 9.8 / 20.0;
      else {
        const int l = (i - 6) / 3;
        const double n = l == 0 ? nz[0] : (l == 1 ? nz[1] : (l == 2 ? nz[2] : nz[3]));
        qd = n * dt * a.prm.process_noise_pfoot;
      }
      v = v + qd;
    }
    Pb[t] = v;
  }
  {
    const int r = lane < NY ? lane : NY - 1;
    const int l = r < 24 ? (r % 12) / 3 : r - 24;
    const int k = r % 3;
    const double cl = l == 0 ? c[0] : (l == 1 ? c[1] : (l == 2 ? c[2] : c[3]));
    const double *f = fk + 3 * l, *fvl = fv + 3 * l;
    double y, yhat;
    if (r < 12) {
      y = Rm[k] * f[0] + Rm[3 + k] * f[1] + Rm[6 + k] * f[2];
      yhat = xbar_of(6 + r) - xbar_of(k);
    } else if (r < 24) {
      double lv[3];  // leg_v = -foot_vel_rel - skew(imu_ang_vel) fk (:122)
      lv[0] = -fvl[0] - (0.0 * f[0] + -om[2] * f[1] + om[1] * f[2]);
      lv[1] = -fvl[1] - (om[2] * f[0] + 0.0 * f[1] + -om[0] * f[2]);
      lv[2] = -fvl[2] - (-om[1] * f[0] + om[0] * f[1] + 0.0 * f[2]);
      const double rl = (cl * Rm[k]) * lv[0] + (cl * Rm[3 + k]) * lv[1] + (cl * Rm[6 + k]) * lv[2];
      y = (1.0 - cl) * xs[3 + k] + rl;  // the prior x, not xbar (:124)
      yhat = xbar_of(3 + k);
    } else {
      y = (1.0 - cl) * (xs[2] + f[2]) + cl * 0.0;  // prior x, body-frame fk z (:127)
      yhat = xbar_of(8 + 3 * l);
    }
    if (lane < NY) es[lane] = y - yhat;
  }
  __syncthreads();

  // 3. row r of S = sym(C Pbar C' + R), lower part, in registers
  const int r = lane < NY ? lane : NY - 1;
  const int rp = c_plus(r), rm = c_minus(r);
  const int rmc = rm < 0 ? 0 : rm;  // in-range address for rows without a minus column
  double arow[NY];
  {
    const int l = r < 24 ? (r % 12) / 3 : r - 24;
    const double n = l == 0 ? nz[0] : (l == 1 ? nz[1] : (l == 2 ? nz[2] : nz[3]));
    double rd;  // R diagonal (:98-106)
    if (r < 12) rd = n * a.prm.sensor_noise_pimu_rel_foot;
    else if (r < 24) rd = n * a.prm.sensor_noise_vimu_rel_foot;
    else rd = a.prm.assume_flat_ground ? n * a.prm.sensor_noise_zfoot : 1e5;
#pragma unroll
    for (int s = 0; s < NY; ++s) {
      const int sp = c_plus(s), sm = c_minus(s);
      // CP[r][k] = Pbar[rp][k] - Pbar[rm][k];  M[r][s] = CP[r][sp] - CP[r][sm]
      double cps = Pb[rp * NX + sp];
      if (rm >= 0) cps = cps - Pb[rmc * NX + sp];
      double mrs = cps;
      // CP[s][k] = Pbar[sp][k] - Pbar[sm][k];  M[s][r] = CP[s][rp] - CP[s][rm]
      double csp = Pb[sp * NX + rp];
      double csm = Pb[sp * NX + rmc];
      if (sm >= 0) {
        double cpm = Pb[rp * NX + sm];
        if (rm >= 0) cpm = cpm - Pb[rmc * NX + sm];
        mrs = cps - cpm;
        csp = csp - Pb[sm * NX + rp];
        csm = csm - Pb[sm * NX + rmc];
      }
      const double msr = (rm >= 0) ? csp - csm : csp;
      const double v = (s == r) ? mrs + rd : 0.5 * (mrs + msr);
      arow[s] = (s <= r) ? v : 0.0;
      sched_fence();
    }
  }
  __syncthreads();  // the dense prior P under L is dead (read in step 2 only)

  // 4. Cholesky-Crout, S = L L'; lane r owns row r, column k published per step
#pragma unroll
  for (int k = 0; k < NY; ++k) {
    double v = arow[k];
#pragma unroll
    for (int j = 0; j < k; ++j) v = v - arow[j] * Lp[k * (k + 1) / 2 + j];
    const double vk = __shfl(v, k, GW);
    const double d = sqrt(vk);
    arow[k] = (r == k) ? d : v / d;
    if (lane < NY && r >= k) Lp[r * (r + 1) / 2 + k] = arow[k];
    __syncthreads();
  }

  // 5. W = L^-1 [C Pbar | e], one column per lane
  const int jc = lane < NW ? lane : NW - 1;
  const int jp = jc < NX ? jc : NX - 1;
  double w[NY];
#pragma unroll
  for (int q = 0; q < NY; ++q) {
    const int qp = c_plus(q), qm = c_minus(q);
    double v = Pb[qp * NX + jp];
    if (qm >= 0) v = v - Pb[qm * NX + jp];
    w[q] = (jc < NX) ? v : es[q];
  }
#pragma unroll
  for (int q = 0; q < NY; ++q) {
    double t = w[q];
#pragma unroll
    for (int k = 0; k < q; ++k) t = t - Lp[q * (q + 1) / 2 + k] * w[k];
    w[q] = t / Lp[q * (q + 1) / 2 + q];
    sched_fence();
  }

  // 6. W beside Pbar (L is dead)
  const int ip = lane < NX ? lane : NX - 1;
  const double xb = xbs[ip];
  __syncthreads();
  double *Wl = sh + L_OFF;
  if (lane < NW) {
#pragma unroll
    for (int q = 0; q < NY; ++q) Wl[q * NW + lane] = w[q];
  }
  __syncthreads();

  // 7. x = xbar + W' z,  P = sym(Pbar - W'W) in place: lane i owns the pairs
  //    {i, i + d}, d = 0..9 (mod 18), which no other lane reads or writes
  double xn = 0.0;
#pragma unroll
  for (int q = 0; q < NY; ++q) xn = xn + w[q] * Wl[q * NW + NX];
  xn = xb + xn;
  if (lane < NX) xs[lane] = xn;
#pragma unroll 1
  for (int d = 0; d < 10; ++d) {
    int j = ip + d;
    j = j >= NX ? j - NX : j;
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < NY; ++q) s = s + w[q] * Wl[q * NW + j];
    const double v = 0.5 * ((Pb[ip * NX + j] - s) + (Pb[j * NX + ip] - s));
    if (lane < NX && (d < 9 || lane < 9)) {
      Pb[ip * NX + j] = v;
      Pb[j * NX + ip] = v;
    }
  }
  __syncthreads();

  // 8. drift reduction (:143-147) and the stores
  const double det = Pb[0] * Pb[NX + 1] - Pb[NX] * Pb[1];
  const bool drift = det > 1e-6;
  if (!active) return;
  for (int t = lane; t < NPK; t += GW) {
    int i, j;
    tri_decode(t, i, j);
    double v = Pb[i * NX + j];
    if (drift) {
      if (i < 2) v = v / 10.0;
      else if (j < 2) v = 0.0;
    }
    wsr[NX + t] = v;
  }
  if (lane < NX) wsr[lane] = xs[lane];
  if (lane < 3) a.root_pos[rb * 3 + lane] = xs[lane];
  else if (lane < 6) a.root_lin_vel[rb * 3 + (lane - 3)] = xs[lane];
  if (a.contacts && lane < 4) {
    const double cl = lane == 0 ? c[0] : (lane == 1 ? c[1] : (lane == 2 ? c[2] : c[3]));
    a.contacts[rb * 4 + lane] = (cl < 0.5) ? 0 : 1;  // :151-157
  }
}

// init_state (:55-68): P = 3 I, x = (0, 0, 0.09 | R fk_i + pos)
__global__ __launch_bounds__(256) void a1_ekf_init_kernel(int64_t n, double *ws,
                                                          const double *__restrict__ rot,
                                                          const double *__restrict__ fk) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const int64_t b = g / WSD;
  const int t = (int)(g - b * WSD);
  double v = 0.0;
  if (t < NX) {
    const int k = t % 3;
    const double x0 = (k == 2) ? 0.09 : 0.0;
    if (t < 3) v = x0;
    else if (t >= 6) {
      const double *R = rot + b * 9, *f = fk + b * 12 + 3 * ((t - 6) / 3);
      v = (R[k] * f[0] + R[3 + k] * f[1] + R[6 + k] * f[2]) + x0;
    }
  } else if (t < NX + NPK) {
    int i, j;
    tri_decode(t - NX, i, j);
    v = (i == j) ? 3.0 : 0.0;
  }
  ws[g] = v;
}

// dense x(18) | P(18x18) <-> workspace record; set reads P's lower triangle
__global__ __launch_bounds__(256) void a1_ekf_get_kernel(int64_t n, const double *__restrict__ ws,
                                                         double *x, double *P) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const int64_t b = g / (NX * NX);
  const int t = (int)(g - b * (NX * NX));
  const int c = t / NX, r = t - c * NX;
  const int i = r > c ? r : c, j = r > c ? c : r;
  P[g] = ws[b * WSD + NX + i * (i + 1) / 2 + j];
  if (t < NX) x[b * NX + t] = ws[b * WSD + t];
}

__global__ __launch_bounds__(256) void a1_ekf_set_kernel(int64_t n, double *ws,
                                                         const double *__restrict__ x,
                                                         const double *__restrict__ P) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const int64_t b = g / WSD;
  const int t = (int)(g - b * WSD);
  double v = 0.0;
  if (t < NX) v = x[b * NX + t];
  else if (t < NX + NPK) {
    int i, j;
    tri_decode(t - NX, i, j);
    v = P[b * (NX * NX) + j * NX + i];  // column-major (i, j), i >= j
  }
  ws[g] = v;
}

constexpr int64_t kMaxBatch = (int64_t)1 << 30;

}  // namespace
}  // namespace qloco

using namespace qloco;

extern "C" void qloco_a1_kin_params_default(qloco_a1_kin_params *p) {
  if (!p) return;
  // GazeboA1ROS.cpp:79-101, legs FL, FR, RL, RR
  const double ox[4] = {0.1805, 0.1805, -0.1805, -0.1805};
  const double oy[4] = {0.047, -0.047, 0.047, -0.047};
  const double mo[4] = {0.0838, -0.0838, 0.0838, -0.0838};
  for (int l = 0; l < 4; ++l) {
    p->rho_fix[l][0] = ox[l];
    p->rho_fix[l][1] = oy[l];
    p->rho_fix[l][2] = mo[l];
    p->rho_fix[l][3] = 0.21;
    p->rho_fix[l][4] = 0.21;
    for (int k = 0; k < 3; ++k) p->rho_opt[l][k] = 0.0;
  }
}

extern "C" int qloco_a1_leg_kin(const qloco_a1_kin_params *prm, int64_t batch,
                                const double *joint_pos, const double *joint_vel,
                                const double *root_quat, const double *root_pos,
                                const double *root_lin_vel, double *foot_pos_rel, double *j_foot,
                                double *foot_vel_rel, double *root_rot_mat, double *root_euler,
                                double *root_rot_mat_z, double *foot_pos_abs, double *foot_vel_abs,
                                double *foot_pos_world, double *foot_vel_world, void *stream) {
  if (!prm || batch <= 0 || batch > kMaxBatch || !joint_pos || !joint_vel || !root_quat ||
      !foot_pos_rel || (foot_pos_world && !root_pos) || (foot_vel_world && !root_lin_vel))
    return QLOCO_ERR_ARG;
  KinArgs a;
  a.prm = *prm;
  a.n = batch * 4;
  a.joint_pos = joint_pos;
  a.joint_vel = joint_vel;
  a.root_quat = root_quat;
  a.root_pos = root_pos;
  a.root_lin_vel = root_lin_vel;
  a.foot_pos_rel = foot_pos_rel;
  a.j_foot = j_foot;
  a.foot_vel_rel = foot_vel_rel;
  a.root_rot_mat = root_rot_mat;
  a.root_euler = root_euler;
  a.root_rot_mat_z = root_rot_mat_z;
  a.foot_pos_abs = foot_pos_abs;
  a.foot_vel_abs = foot_vel_abs;
  a.foot_pos_world = foot_pos_world;
  a.foot_vel_world = foot_vel_world;
  hipLaunchKernelGGL(a1_leg_kin_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, a);
  QLOCO_HIP_CHECK(hipGetLastError(), "a1_leg_kin_kernel launch");
  return QLOCO_OK;
}

extern "C" void qloco_a1_ekf_params_default(qloco_a1_ekf_params *p) {
  if (!p) return;
  p->process_noise_pimu = 0.01;  // A1BasicEKF.h:16-21
  p->process_noise_vimu = 0.01;
  p->process_noise_pfoot = 0.01;
  p->sensor_noise_pimu_rel_foot = 0.001;
  p->sensor_noise_vimu_rel_foot = 0.1;
  p->sensor_noise_zfoot = 0.001;
  p->assume_flat_ground = 1;  // the default-constructed member (GazeboA1ROS.h:160)
  for (int k = 0; k < 7; ++k) p->reserved[k] = 0;
}

extern "C" int64_t qloco_a1_ekf_workspace_bytes(int64_t batch) {
  if (batch <= 0 || batch > kMaxBatch) return -1;
  return batch * (int64_t)WSD * (int64_t)sizeof(double);
}

extern "C" int qloco_a1_ekf_init(const qloco_a1_ekf_params *prm, int64_t batch, void *workspace,
                                 const double *root_rot_mat, const double *foot_pos_rel,
                                 void *stream) {
  if (!prm || batch <= 0 || batch > kMaxBatch || !workspace || !root_rot_mat || !foot_pos_rel)
    return QLOCO_ERR_ARG;
  const int64_t n = batch * WSD;
  hipLaunchKernelGGL(a1_ekf_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, n, (double *)workspace, root_rot_mat, foot_pos_rel);
  QLOCO_HIP_CHECK(hipGetLastError(), "a1_ekf_init_kernel launch");
  return QLOCO_OK;
}

extern "C" int qloco_a1_ekf_update(const qloco_a1_ekf_params *prm, int64_t batch, void *workspace,
                                   const double *dt, const int32_t *movement_mode,
                                   const double *root_rot_mat, const double *imu_acc,
                                   const double *imu_ang_vel, const double *foot_pos_rel,
                                   const double *foot_vel_rel, const double *foot_force,
                                   double *root_pos, double *root_lin_vel,
                                   uint8_t *estimated_contacts, void *stream) {
  if (!prm || batch <= 0 || batch > kMaxBatch || !workspace || !dt || !movement_mode ||
      !root_rot_mat || !imu_acc || !imu_ang_vel || !foot_pos_rel || !foot_vel_rel || !foot_force ||
      !root_pos || !root_lin_vel)
    return QLOCO_ERR_ARG;
  EkfArgs a;
  a.prm = *prm;
  a.batch = batch;
  a.ws = (double *)workspace;
  a.dt = dt;
  a.mode = movement_mode;
  a.rot = root_rot_mat;
  a.acc = imu_acc;
  a.omega = imu_ang_vel;
  a.fk = foot_pos_rel;
  a.fvel = foot_vel_rel;
  a.force = foot_force;
  a.root_pos = root_pos;
  a.root_lin_vel = root_lin_vel;
  a.contacts = estimated_contacts;
  hipLaunchKernelGGL(a1_ekf_update_kernel, dim3((unsigned)((batch + RPB - 1) / RPB)),
                     dim3(GW * RPB), 0, (hipStream_t)stream, a);
  QLOCO_HIP_CHECK(hipGetLastError(), "a1_ekf_update_kernel launch");
  return QLOCO_OK;
}

extern "C" int qloco_a1_ekf_get_state(int64_t batch, const void *workspace, double *x, double *P,
                                      void *stream) {
  if (batch <= 0 || batch > kMaxBatch || !workspace || !x || !P) return QLOCO_ERR_ARG;
  const int64_t n = batch * NX * NX;
  hipLaunchKernelGGL(a1_ekf_get_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, n, (const double *)workspace, x, P);
  QLOCO_HIP_CHECK(hipGetLastError(), "a1_ekf_get_kernel launch");
  return QLOCO_OK;
}

extern "C" int qloco_a1_ekf_set_state(int64_t batch, void *workspace, const double *x,
                                      const double *P, void *stream) {
  if (batch <= 0 || batch > kMaxBatch || !workspace || !x || !P) return QLOCO_ERR_ARG;
  const int64_t n = batch * WSD;
  hipLaunchKernelGGL(a1_ekf_set_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, n, (double *)workspace, x, P);
  QLOCO_HIP_CHECK(hipGetLastError(), "a1_ekf_set_kernel launch");
  return QLOCO_OK;
}

// qloco_a1ctrl.hip -- batched A1 gait plan, swing-leg control, terrain pitch
// and joint torques, fp64 like the reference (include/qloco.h section 13).
//
// Covers, of unitree_ros/a1_cpp_open_source/src/A1RobotControl.cpp:
//   a1_plan_swing_kernel   update_plan (:149-207) then generate_swing_legs_ctrl
//                          (:209-292), one leg per lane (legs FL, FR, RL, RR)
//   a1_terrain_kernel      the stance_leg_control_type == 1 preamble of
//                          compute_grf (:341-380) with compute_walking_surface
//                          (:604-620), Utils::pseudo_inverse and
//                          Utils::cal_dihedral_angle (Utils.cpp:44-62), one
//                          robot per lane
//   a1_torque_kernel       compute_joint_torques (:294-324), one leg per lane
//
// Workspace.  Every per-robot member is a field of a dense record of
// QLOCO_A1_CTRL_STATE doubles (the order get_state / set_state use, listed in
// qloco.h); on the device field f of length len(f) starting at record offset
// o(f) lives at ws[o(f) * B + b * len(f) + j], i.e. field-major: consecutive
// lanes touch consecutive addresses for every member.  Flags, ring fill counts
// and heads are stored as doubles.  The moving-window rings are slot-major:
// slot s of the twelve recent-contact filters of robot b is the 12-vector at
// ws[(RC_RING + 12 s) * B + 12 b], so lanes whose heads agree (robots reset
// together) read and write one contiguous span, and lanes whose heads differ
// still touch one 24-byte piece each -- never more sectors than a per-robot
// ring would.  A filter update reads the oldest slot
// and writes the new one: O(1), independent of the window length.  The x, y
// and z filters of a leg always advance together, so they share one fill
// count and one head.
//
// Every loop has a fixed trip count.  NaN and inf inputs propagate; the only
// data-dependent branches are the reference's own tests.  Ring indices read
// from the workspace are clamped into the ring before use.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "qloco.h"
#include "qloco_common.hpp"

namespace qloco {
namespace {

constexpr int REC = QLOCO_A1_CTRL_STATE;
constexpr int RCW = QLOCO_A1_CTRL_RC_WINDOW_MAX;   // 60
constexpr int TEW = QLOCO_A1_CTRL_TER_WINDOW_MAX;  // 100
// record offsets (doubles)
constexpr int O_GC = 0, O_PLAN = 4, O_EARLY = 8, O_CONT = 12;
constexpr int O_START = 16, O_REL_LAST = 28, O_TGT_LAST = 40, O_TGT_REL = 52, O_RECENT = 64;
constexpr int O_FKIN = 76, O_JT = 88, O_MPC = 100, O_TERRAIN = 101;
constexpr int O_RC_FILL = 102, O_RC_HEAD = 106, O_RC_SUM = 110, O_RC_CORR = 122;
constexpr int O_TE_FILL = 134, O_TE_HEAD = 135, O_TE_SUM = 136, O_TE_CORR = 137;
constexpr int O_RC_RING = 138, O_TE_RING = O_RC_RING + 12 * RCW;
static_assert(O_TE_RING + TEW == REC, "record length");

// record position t -> (field start, field length)
__host__ __device__ inline void field_of(int t, int &o, int &len) {
  if (t < O_START) { o = t & ~3; len = 4; }
  else if (t < O_MPC) { o = O_START + 12 * ((t - O_START) / 12); len = 12; }
  else if (t < O_RC_FILL) { o = t; len = 1; }
  else if (t < O_RC_SUM) { o = O_RC_FILL + 4 * ((t - O_RC_FILL) / 4); len = 4; }
  else if (t < O_TE_FILL) { o = O_RC_SUM + 12 * ((t - O_RC_SUM) / 12); len = 12; }
  else if (t < O_RC_RING) { o = t; len = 1; }
  else if (t < O_TE_RING) { o = O_RC_RING + 12 * ((t - O_RC_RING) / 12); len = 12; }
  else { o = t; len = 1; }
}

// MovingWindowFilter::UpdateNeumaierSum (utils/filter.hpp:53-62): the branch
// compares |sum| and |value|
__device__ __forceinline__ void neumaier(double &sum, double &corr, double value) {
  const double new_sum = sum + value;
  if (fabs(sum) >= fabs(value)) corr = corr + ((sum - new_sum) + value);
  else corr = corr + ((value - new_sum) + sum);
  sum = new_sum;
}

__device__ __forceinline__ int ring_index(double v, int hi) {  // clamp into [0, hi]
  int i = (int)v;
  i = i < 0 ? 0 : i;
  return i > hi ? hi : i;
}

// BezierUtils::bezier_curve (Utils.cpp:100-107): the degree-4 Bernstein sum
// y += c_i * t^i * (1 - t)^(4 - i) * P_i, i = 0..4, in that order; the powers
// by repeated multiplication where the reference calls std::pow (rounding
// parity, tests/a1_ctrl_ref.py)
__device__ __forceinline__ double bezier4(double t, const double P[5]) {
  const double u = 1 - t;
  const double t2 = t * t, t3 = t2 * t, t4 = t3 * t;
  const double u2 = u * u, u3 = u2 * u, u4 = u3 * u;
  double y = 0;
  y = y + 1.0 * 1.0 * u4 * P[0];
  y = y + 4.0 * t * u3 * P[1];
  y = y + 6.0 * t2 * u2 * P[2];
  y = y + 4.0 * t3 * u * P[3];
  y = y + 1.0 * t4 * 1.0 * P[4];
  return y;
}

struct PlanArgs {
  qloco_a1_ctrl_params prm;
  int64_t batch;
  double *ws;
  const double *dt;
  const int32_t *mode;
  const double *root_pos, *root_lin_vel, *root_lin_vel_d, *rot, *rot_z, *foot_pos_abs, *foot_force;
  uint8_t *contacts, *plan_contacts, *early_contacts;
  double *gait_counter, *tgt_rel, *tgt_abs, *tgt_world, *foot_pos_cur, *fkin, *recent;
};

__global__ __launch_bounds__(256) void a1_plan_swing_kernel(PlanArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t B = a.batch;
  if (i >= 4 * B) return;
  const int64_t b = i >> 2;
  const int leg = (int)(i & 3);
  double *ws = a.ws;
  const double dt = a.dt[b];
  const int mode = a.mode[b];
  const double cpg = a.prm.counter_per_gait, cps = a.prm.counter_per_swing;
  const double speed = a.prm.gait_counter_speed[leg];

  // ---- update_plan (:149-166).  Standstill sets every plan_contact and
  // resets the counters on every tick.  Walking: the counter advances by
  // gait_counter_speed and then takes std::fmod with counter_per_gait; the leg
  // is in STANCE while gait_counter <= counter_per_swing, despite the name.
  double gc = ws[O_GC * B + i];
  bool plan;
  if (!mode) {
    plan = true;
    gc = a.prm.gait_counter_reset[leg];
  } else {
    gc = gc + speed;
    gc = fmod(gc, cpg);
    plan = gc <= cps;
  }
  ws[O_GC * B + i] = gc;
  ws[O_PLAN * B + i] = plan ? 1.0 : 0.0;

  // ---- Raibert heuristic (:169-201).  The velocity is rotated into the
  // root_rot_mat_z' frame.  default_foot_pos(2) is entry 2 of the 3x4 matrix
  // in column-major linear order, FL's z, for every leg.  Clamp +-limit, then
  // root_rot_mat * target_rel and + root_pos.
  const double *Rz = a.rot_z + 9 * b, *Rm = a.rot + 9 * b;
  const double *v = a.root_lin_vel + 3 * b, *vd = a.root_lin_vel_d + 3 * b;
  const double lvx = Rz[0] * v[0] + Rz[1] * v[1] + Rz[2] * v[2];
  const double lvy = Rz[3] * v[0] + Rz[4] * v[1] + Rz[5] * v[2];
  const double k1 = sqrt(fabs(a.prm.default_foot_pos[2]) / 9.8);
  const double k2 = ((cps / speed) * a.prm.control_dt) / 2.0;
  double dx = k1 * (lvx - vd[0]) + k2 * vd[0];
  double dy = k1 * (lvy - vd[1]) + k2 * vd[1];
  if (dx < -a.prm.foot_delta_x_limit) dx = -a.prm.foot_delta_x_limit;
  if (dx > a.prm.foot_delta_x_limit) dx = a.prm.foot_delta_x_limit;
  if (dy < -a.prm.foot_delta_y_limit) dy = -a.prm.foot_delta_y_limit;
  if (dy > a.prm.foot_delta_y_limit) dy = a.prm.foot_delta_y_limit;
  double tr[3];
  tr[0] = a.prm.default_foot_pos[3 * leg] + dx;
  tr[1] = a.prm.default_foot_pos[3 * leg + 1] + dy;
  tr[2] = a.prm.default_foot_pos[3 * leg + 2];
  double ta[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ta[k] = Rm[k] * tr[0] + Rm[3 + k] * tr[1] + Rm[6 + k] * tr[2];
    ws[O_TGT_REL * B + 3 * i + k] = tr[k];
    if (a.tgt_rel) a.tgt_rel[3 * i + k] = tr[k];
    if (a.tgt_abs) a.tgt_abs[3 * i + k] = ta[k];
    if (a.tgt_world) a.tgt_world[3 * i + k] = ta[k] + a.root_pos[3 * b + k];
  }

  // ---- generate_swing_legs_ctrl (:209-258).  state.joint_torques is zeroed
  // (:210), so the value the NaN guard of compute_joint_torques holds is zero
  // whenever this call ran since the last torque call.
  const double *fa = a.foot_pos_abs + 3 * i;
  double cur[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ws[O_JT * B + 3 * i + k] = 0.0;
    cur[k] = Rz[3 * k] * fa[0] + Rz[3 * k + 1] * fa[1] + Rz[3 * k + 2] * fa[2];
  }
  // Spline time in float32 (:240): float(gc - cps) / float(cps), passed on as
  // float t.  Stance feet refresh foot_pos_start every tick.
  float st = 0.0f;
  double s[3];
  if (gc <= cps) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      s[k] = cur[k];
      ws[O_START * B + 3 * i + k] = cur[k];
    }
  } else {
    st = (float)(gc - cps) / (float)cps;
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = ws[O_START * B + 3 * i + k];
  }
  // get_foot_pos_curve (Utils.cpp:64-97): control points {s, s, f, f, f}; z
  // adds the clearances (float literals widened to double); the terrain
  // argument is always 0.0 (:246), so 0.5 * sin(0.0) = 0.0 is added to it.
  const double t = (double)st;
  double tgt[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double P[5] = {s[k], s[k], tr[k], tr[k], tr[k]};
    if (k == 2) {
      P[1] = P[1] + a.prm.foot_swing_clearance1;
      P[2] = P[2] + (a.prm.foot_swing_clearance2 + 0.5 * 0.0);
    }
    tgt[k] = bezier4(t, P);
  }
  // Foot velocities: finite differences over the caller's dt against the
  // *_last_time members (zero after reset; dt = 0 gives inf / NaN as in the
  // reference).  foot_forces_kin = kp o e_p + kd o e_v, for stance legs too.
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double vc = (cur[k] - ws[O_REL_LAST * B + 3 * i + k]) / dt;
    const double vt = (tgt[k] - ws[O_TGT_LAST * B + 3 * i + k]) / dt;
    ws[O_REL_LAST * B + 3 * i + k] = cur[k];
    ws[O_TGT_LAST * B + 3 * i + k] = tgt[k];
    const double ep = tgt[k] - cur[k], ev = vt - vc;
    const double f = ep * a.prm.kp_foot[3 * leg + k] + ev * a.prm.kd_foot[3 * leg + k];
    ws[O_FKIN * B + 3 * i + k] = f;
    if (a.fkin) a.fkin[3 * i + k] = f;
    if (a.foot_pos_cur) a.foot_pos_cur[3 * i + k] = cur[k];
  }

  // ---- early contact (:264-276): the flag clears while gc <= 1.5 cps; it
  // sets when the leg is not planned, gc > 1.5 cps and foot_force >
  // FOOT_FORCE_LOW.  contacts = plan || early.
  bool early = ws[O_EARLY * B + i] != 0.0;
  if (gc <= cps * 1.5) early = false;
  if (!plan && (gc > cps * 1.5) && (a.foot_force[i] > a.prm.foot_force_low)) early = true;
  const bool contact = plan || early;
  ws[O_EARLY * B + i] = early ? 1.0 : 0.0;
  ws[O_CONT * B + i] = contact ? 1.0 : 0.0;
  a.contacts[i] = contact ? 1 : 0;
  if (a.plan_contacts) a.plan_contacts[i] = plan ? 1 : 0;
  if (a.early_contacts) a.early_contacts[i] = early ? 1 : 0;
  if (a.gait_counter) a.gait_counter[i] = gc;

  // ---- recent-contact filters (:279-286, filter.hpp:26-39): they advance
  // only for legs in contact; the average divides by the window size even
  // while the ring is filling.
  if (contact) {
    const int W = a.prm.recent_contact_window;
    int fill = ring_index(ws[O_RC_FILL * B + i], W);
    int head = ring_index(ws[O_RC_HEAD * B + i], W - 1);
    const bool full = fill >= W;
    int slot = head + fill;
    slot = slot >= W ? slot - W : slot;
    slot = full ? head : slot;
    double *ring = ws + (int64_t)(O_RC_RING + 12 * slot) * B + 3 * i;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double sum = ws[O_RC_SUM * B + 3 * i + k], corr = ws[O_RC_CORR * B + 3 * i + k];
      if (full) neumaier(sum, corr, -ring[k]);
      neumaier(sum, corr, fa[k]);
      ring[k] = fa[k];
      ws[O_RC_SUM * B + 3 * i + k] = sum;
      ws[O_RC_CORR * B + 3 * i + k] = corr;
      ws[O_RECENT * B + 3 * i + k] = (sum + corr) / (double)W;
    }
    if (full) head = head + 1 == W ? 0 : head + 1;
    else fill = fill + 1;
    ws[O_RC_FILL * B + i] = (double)fill;
    ws[O_RC_HEAD * B + i] = (double)head;
  }
  if (a.recent) {
#pragma unroll
    for (int k = 0; k < 3; ++k) a.recent[3 * i + k] = ws[O_RECENT * B + 3 * i + k];
  }
}

// ------------------------------------------------------------------- terrain
struct TerrainArgs {
  qloco_a1_ctrl_params prm;
  int64_t batch;
  double *ws;
  const double *root_pos;
  double *root_euler_d, *angle, *surf_coef;
};

// One cyclic-Jacobi rotation of the symmetric 3x3 A (full storage) on the
// pair (p, q), r the third index; V accumulates the eigenvectors by columns.
template <int p, int q, int r>
__device__ __forceinline__ void jacobi_rot(double A[3][3], double V[3][3]) {
  const double apq = A[p][q];
  const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
  const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double t = (apq == 0.0) ? 0.0 : tt;  // a zero off-diagonal entry needs no rotation
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  const double app = A[p][p], aqq = A[q][q], arp = A[r][p], arq = A[r][q];
  A[p][p] = app - t * apq;
  A[q][q] = aqq + t * apq;
  A[p][q] = A[q][p] = 0.0;
  A[r][p] = A[p][r] = c * arp - s * arq;
  A[r][q] = A[q][r] = s * arp + c * arq;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double vp = V[k][p], vq = V[k][q];
    V[k][p] = c * vp - s * vq;
    V[k][q] = s * vp + c * vq;
  }
}

constexpr int kJacobiSweeps = 8;

__global__ __launch_bounds__(256) void a1_terrain_kernel(TerrainArgs a) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t B = a.batch;
  if (b >= B) return;
  double *ws = a.ws;
  double x[4], y[4], z[4];
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    x[l] = ws[O_RECENT * B + 12 * b + 3 * l];
    y[l] = ws[O_RECENT * B + 12 * b + 3 * l + 1];
    z[l] = ws[O_RECENT * B + 12 * b + 3 * l + 2];
  }
  // compute_walking_surface (:604-620): W = [1, x_i, y_i], a = pinv(W'W) W' z
  double A[3][3], V[3][3];
  {
    double s1 = 0, sx = 0, sy = 0, sxx = 0, sxy = 0, syy = 0;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      s1 = s1 + 1.0 * 1.0;
      sx = sx + 1.0 * x[l];
      sy = sy + 1.0 * y[l];
      sxx = sxx + x[l] * x[l];
      sxy = sxy + x[l] * y[l];
      syy = syy + y[l] * y[l];
    }
    A[0][0] = s1, A[0][1] = A[1][0] = sx, A[0][2] = A[2][0] = sy;
    A[1][1] = sxx, A[1][2] = A[2][1] = sxy, A[2][2] = syy;
  }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) V[r][c] = r == c ? 1.0 : 0.0;
  // W'W is symmetric PSD: its eigen-decomposition (fixed-sweep cyclic Jacobi)
  // is its SVD.  pseudo_inverse (Utils.cpp:44-52) keeps the singular values
  // above eps * 3 * sigma_max and zeroes the others.
#pragma unroll 1
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
    jacobi_rot<0, 1, 2>(A, V);
    jacobi_rot<0, 2, 1>(A, V);
    jacobi_rot<1, 2, 0>(A, V);
  }
  const double l0 = fabs(A[0][0]), l1 = fabs(A[1][1]), l2 = fabs(A[2][2]);
  double lmax = l0 > l1 ? l0 : l1;
  lmax = lmax > l2 ? lmax : l2;
  const double tol = 2.220446049250313e-16 * 3.0 * lmax;
  double inv[3];
  inv[0] = l0 > tol ? 1.0 / A[0][0] : 0.0;
  inv[1] = l1 > tol ? 1.0 / A[1][1] : 0.0;
  inv[2] = l2 > tol ? 1.0 / A[2][2] : 0.0;
  double Pi[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      Pi[r][c] = (V[r][0] * inv[0]) * V[c][0] + (V[r][1] * inv[1]) * V[c][1] + (V[r][2] * inv[2]) * V[c][2];
  double co[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    double acc = 0;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const double m = Pi[r][0] * 1.0 + Pi[r][1] * x[l] + Pi[r][2] * y[l];  // (pinv W')(r, l)
      acc = acc + m * z[l];
    }
    co[r] = acc;
  }
  // surf_coef = (a1, a2, -1); cal_dihedral_angle against (0, 0, 1):
  // acos(|n1.n2| / (|n1| |n2|))
  const double sc[3] = {co[1], co[2], -1.0};
  const double dot = fabs(0.0 * sc[0] + 0.0 * sc[1] + 1.0 * sc[2]);
  const double den = sqrt(0.0 * 0.0 + 0.0 * 0.0 + 1.0 * 1.0) * sqrt(sc[0] * sc[0] + sc[1] * sc[1] + sc[2] * sc[2]);
  const double dihedral = acos(dot / den);
  // The terrain filter is fed only when root_pos[2] > 0.1 (:347); otherwise
  // the angle is 0 and the filter is untouched.
  double angle = 0.0;
  if (a.root_pos[3 * b + 2] > 0.1) {
    const int W = a.prm.terrain_window;
    int fill = ring_index(ws[O_TE_FILL * B + b], W);
    int head = ring_index(ws[O_TE_HEAD * B + b], W - 1);
    const bool full = fill >= W;
    int slot = head + fill;
    slot = slot >= W ? slot - W : slot;
    slot = full ? head : slot;
    double *ring = ws + (int64_t)(O_TE_RING + slot) * B + b;
    double sum = ws[O_TE_SUM * B + b], corr = ws[O_TE_CORR * B + b];
    if (full) neumaier(sum, corr, -ring[0]);
    neumaier(sum, corr, dihedral);
    ring[0] = dihedral;
    if (full) head = head + 1 == W ? 0 : head + 1;
    else fill = fill + 1;
    ws[O_TE_SUM * B + b] = sum;
    ws[O_TE_CORR * B + b] = corr;
    ws[O_TE_FILL * B + b] = (double)fill;
    ws[O_TE_HEAD * B + b] = (double)head;
    angle = (sum + corr) / (double)W;
  }
  // clamp +-0.5 (:353-358); root_euler_d[1] = -angle if z_FL + z_FR - z_RL -
  // z_RR > 0.05, else +angle (:361-368)
  if (angle > 0.5) angle = 0.5;
  if (angle < -0.5) angle = -0.5;
  const double frd = z[0] + z[1] - z[2] - z[3];
  a.root_euler_d[3 * b + 1] = (frd > 0.05) ? -angle : angle;
  ws[O_TERRAIN * B + b] = angle;
  a.angle[b] = angle;
  if (a.surf_coef) {
#pragma unroll
    for (int k = 0; k < 3; ++k) a.surf_coef[3 * b + k] = sc[k];
  }
}

// -------------------------------------------------------------------- torques
struct TorqueArgs {
  qloco_a1_ctrl_params prm;
  int64_t batch;
  double *ws;
  const double *j_foot, *grf;
  double *tau;
};

__device__ __forceinline__ void swap_if(bool c, double &x, double &y) {
  const double tx = x, ty = y;
  x = c ? ty : tx;
  y = c ? tx : ty;
}

// jac.lu().solve(f): partial-pivot LU of the column-major 3x3 J (first largest
// |entry| of the column on ties, no division by a zero pivot), then the
// permuted unit-lower and upper solves, column by column
__device__ __forceinline__ void lu_solve3(const double J[9], const double f[3], double x[3]) {
  double a00 = J[0], a10 = J[1], a20 = J[2], a01 = J[3], a11 = J[4], a21 = J[5], a02 = J[6], a12 = J[7], a22 = J[8];
  double y0 = f[0], y1 = f[1], y2 = f[2];
  // column 0
  {
    const bool p1 = fabs(a10) > fabs(a00);
    const double m01 = p1 ? fabs(a10) : fabs(a00);
    const bool p2 = fabs(a20) > m01;
    const double big = p2 ? fabs(a20) : m01;
    const bool s1 = p1 && !p2;  // swap rows 0, 1
    swap_if(s1, a00, a10), swap_if(s1, a01, a11), swap_if(s1, a02, a12), swap_if(s1, y0, y1);
    swap_if(p2, a00, a20), swap_if(p2, a01, a21), swap_if(p2, a02, a22), swap_if(p2, y0, y2);
    if (big != 0.0) {
      a10 = a10 / a00;
      a20 = a20 / a00;
    }
    a11 = a11 - a10 * a01, a12 = a12 - a10 * a02;
    a21 = a21 - a20 * a01, a22 = a22 - a20 * a02;
  }
  // column 1
  {
    const bool p2 = fabs(a21) > fabs(a11);
    const double big = p2 ? fabs(a21) : fabs(a11);
    swap_if(p2, a10, a20), swap_if(p2, a11, a21), swap_if(p2, a12, a22), swap_if(p2, y1, y2);
    if (big != 0.0) a21 = a21 / a11;
    a22 = a22 - a21 * a12;
  }
  y1 = y1 - a10 * y0;
  y2 = y2 - a20 * y0;
  y2 = y2 - a21 * y1;
  x[2] = y2 / a22;
  y0 = y0 - a02 * x[2];
  y1 = y1 - a12 * x[2];
  x[1] = y1 / a11;
  y0 = y0 - a01 * x[1];
  x[0] = y0 / a00;
}

__global__ __launch_bounds__(256) void a1_torque_kernel(TorqueArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t B = a.batch;
  if (i >= 4 * B) return;
  const int64_t b = i >> 2;
  const int leg = (int)(i & 3);
  double *ws = a.ws;
  // mpc_init_counter increments first (:297); torques are zero while it is
  // below the hold-off.  The four lanes of a robot sit in one wave and read
  // the counter before lane 0 writes it back (saturating, so it never wraps).
  const double cnt0 = ws[O_MPC * B + b];
  const double cnt = cnt0 < 2147483647.0 ? cnt0 + 1.0 : cnt0;
  const bool contact = ws[O_CONT * B + i] != 0.0;
  double J[9], tau[3], held[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) J[k] = a.j_foot[9 * i + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) held[k] = ws[O_JT * B + 3 * i + k];
  if (leg == 0) ws[O_MPC * B + b] = cnt;
  if (cnt < (double)a.prm.torque_holdoff_ticks) {
#pragma unroll
    for (int k = 0; k < 3; ++k) held[k] = 0.0;
  } else {
    if (contact) {
      // stance leg: J' * (-F_grf)
      const double n0 = -a.grf[3 * i], n1 = -a.grf[3 * i + 1], n2 = -a.grf[3 * i + 2];
#pragma unroll
      for (int k = 0; k < 3; ++k) tau[k] = J[3 * k] * n0 + J[3 * k + 1] * n1 + J[3 * k + 2] * n2;
    } else {
      // swing leg: solve J tau = km o F_kin
      double f[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) f[k] = a.prm.km_foot[k] * ws[O_FKIN * B + 3 * i + k];
      lu_solve3(J, f, tau);
    }
    // gravity compensation on both, then the per-entry NaN guard (:316-322)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double v = tau[k] + a.prm.torques_gravity[3 * leg + k];
      if (!isnan(v)) held[k] = v;
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ws[O_JT * B + 3 * i + k] = held[k];
    a.tau[3 * i + k] = held[k];
  }
}

// ------------------------------------------------------- reset / get / set
__global__ __launch_bounds__(256) void a1_ctrl_reset_kernel(int64_t B, double *ws, double g0,
                                                            double g1, double g2, double g3) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= B * REC) return;
  // A1CtrlStates::reset() and the A1RobotControl constructor: everything zero
  // but the gait counters
  double v = 0.0;
  if (g < 4 * B) {
    const int leg = (int)(g & 3);
    v = leg == 0 ? g0 : (leg == 1 ? g1 : (leg == 2 ? g2 : g3));
  }
  ws[g] = v;
}

template <bool SET>
__global__ __launch_bounds__(256) void a1_ctrl_copy_kernel(int64_t B, double *ws, double *dense) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= B * REC) return;
  const int64_t b = g / REC;
  const int t = (int)(g - b * REC);
  int o, len;
  field_of(t, o, len);
  const int64_t w = (int64_t)o * B + b * len + (t - o);
  if (SET) ws[w] = dense[g];
  else dense[g] = ws[w];
}

constexpr int64_t kMaxBatch = (int64_t)1 << 24;  // 4 * batch * REC stays far below 2^63

bool params_ok(const qloco_a1_ctrl_params *p) {
  return p && p->recent_contact_window >= 1 && p->recent_contact_window <= RCW &&
         p->terrain_window >= 1 && p->terrain_window <= TEW;
}

}  // namespace
}  // namespace qloco

using namespace qloco;

extern "C" void qloco_a1_ctrl_params_default(qloco_a1_ctrl_params *p) {
  if (!p) return;
  p->counter_per_gait = 120 * 2;  // A1CtrlStates.h:23-24
  p->counter_per_swing = 120;
  const double reset[4] = {0, 120, 120, 0};  // gait_counter_reset, gait_type 1 (:319-323)
  // default_foot_pos (:44-46), kp_foot / kd_foot (:104-119), 3x4 col-major
  const double fx[4] = {0.17, 0.17, -0.17, -0.17}, fy[4] = {0.15, -0.15, 0.15, -0.15};
  const double tg[4] = {0.80, -0.80, 0.80, -0.80};  // torques_gravity (:128)
  for (int l = 0; l < 4; ++l) {
    p->gait_counter_speed[l] = 2;  // :102
    p->gait_counter_reset[l] = reset[l];
    p->default_foot_pos[3 * l] = fx[l];
    p->default_foot_pos[3 * l + 1] = fy[l];
    p->default_foot_pos[3 * l + 2] = -0.35;
    p->kp_foot[3 * l] = 300.0;
    p->kp_foot[3 * l + 1] = 400.0;
    p->kp_foot[3 * l + 2] = 400.0;
    for (int k = 0; k < 3; ++k) p->kd_foot[3 * l + k] = 8.0;
    p->torques_gravity[3 * l] = tg[l];
    p->torques_gravity[3 * l + 1] = 0;
    p->torques_gravity[3 * l + 2] = 0;
  }
  p->control_dt = 2.5 / 1000.0;  // MAIN_UPDATE_FREQUENCY / 1000.0 (:328)
  for (int k = 0; k < 3; ++k) p->km_foot[k] = 0.1;  // :121
  p->foot_delta_x_limit = 0.1;  // A1Params.h:44-45
  p->foot_delta_y_limit = 0.1;
  p->foot_force_low = 30.0;             // A1Params.h:38
  p->foot_swing_clearance1 = 0.0f;      // A1Params.h:41-42, float literals
  p->foot_swing_clearance2 = 0.4f;
  p->recent_contact_window = 60;        // A1RobotControl.cpp:53-58
  p->terrain_window = 100;
  p->torque_holdoff_ticks = 10;         // :299
  for (int k = 0; k < 5; ++k) p->reserved[k] = 0;
}

extern "C" int64_t qloco_a1_ctrl_workspace_bytes(int64_t batch) {
  if (batch <= 0 || batch > kMaxBatch) return -1;
  return batch * (int64_t)REC * (int64_t)sizeof(double);
}

extern "C" int qloco_a1_ctrl_reset(const qloco_a1_ctrl_params *prm, int64_t batch, void *workspace,
                                   void *stream) {
  if (!params_ok(prm) || batch <= 0 || batch > kMaxBatch || !workspace) return QLOCO_ERR_ARG;
  const int64_t n = batch * REC;
  hipLaunchKernelGGL(a1_ctrl_reset_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, batch, (double *)workspace, prm->gait_counter_reset[0],
                     prm->gait_counter_reset[1], prm->gait_counter_reset[2],
                     prm->gait_counter_reset[3]);
  QLOCO_HIP_CHECK(hipGetLastError(), "a1_ctrl_reset_kernel launch");
  return QLOCO_OK;
}

extern "C" int qloco_a1_ctrl_plan_swing(
    const qloco_a1_ctrl_params *prm, int64_t batch, void *workspace, const double *dt,
    const int32_t *movement_mode, const double *root_pos, const double *root_lin_vel,
    const double *root_lin_vel_d, const double *root_rot_mat, const double *root_rot_mat_z,
    const double *foot_pos_abs, const double *foot_force, uint8_t *contacts,
    uint8_t *plan_contacts, uint8_t *early_contacts, double *gait_counter,
    double *foot_pos_target_rel, double *foot_pos_target_abs, double *foot_pos_target_world,
    double *foot_pos_cur, double *foot_forces_kin, double *foot_pos_recent_contact, void *stream) {
  if (!params_ok(prm) || batch <= 0 || batch > kMaxBatch || !workspace || !dt || !movement_mode ||
      !root_pos || !root_lin_vel || !root_lin_vel_d || !root_rot_mat || !root_rot_mat_z ||
      !foot_pos_abs || !foot_force || !contacts)
    return QLOCO_ERR_ARG;
  PlanArgs a;
  a.prm = *prm;
  a.batch = batch;
  a.ws = (double *)workspace;
  a.dt = dt;
  a.mode = movement_mode;
  a.root_pos = root_pos;
  a.root_lin_vel = root_lin_vel;
  a.root_lin_vel_d = root_lin_vel_d;
  a.rot = root_rot_mat;
  a.rot_z = root_rot_mat_z;
  a.foot_pos_abs = foot_pos_abs;
  a.foot_force = foot_force;
  a.contacts = contacts;
  a.plan_contacts = plan_contacts;
  a.early_contacts = early_contacts;
  a.gait_counter = gait_counter;
  a.tgt_rel = foot_pos_target_rel;
  a.tgt_abs = foot_pos_target_abs;
  a.tgt_world = foot_pos_target_world;
  a.foot_pos_cur = foot_pos_cur;
  a.fkin = foot_forces_kin;
  a.recent = foot_pos_recent_contact;
  hipLaunchKernelGGL(a1_plan_swing_kernel, dim3((unsigned)((4 * batch + 255) / 256)), dim3(256),
                     0, (hipStream_t)stream, a);
  QLOCO_HIP_CHECK(hipGetLastError(), "a1_plan_swing_kernel launch");
  return QLOCO_OK;
}

extern "C" int qloco_a1_ctrl_terrain(const qloco_a1_ctrl_params *prm, int64_t batch,
                                     void *workspace, const double *root_pos, double *root_euler_d,
                                     double *terrain_pitch_angle, double *surf_coef, void *stream) {
  if (!params_ok(prm) || batch <= 0 || batch > kMaxBatch || !workspace || !root_pos ||
      !root_euler_d || !terrain_pitch_angle)
    return QLOCO_ERR_ARG;
  TerrainArgs a;
  a.prm = *prm;
  a.batch = batch;
  a.ws = (double *)workspace;
  a.root_pos = root_pos;
  a.root_euler_d = root_euler_d;
  a.angle = terrain_pitch_angle;
  a.surf_coef = surf_coef;
  hipLaunchKernelGGL(a1_terrain_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, a);
  QLOCO_HIP_CHECK(hipGetLastError(), "a1_terrain_kernel launch");
  return QLOCO_OK;
}

extern "C" int qloco_a1_ctrl_joint_torques(const qloco_a1_ctrl_params *prm, int64_t batch,
                                           void *workspace, const double *j_foot,
                                           const double *foot_forces_grf, double *joint_torques,
                                           void *stream) {
  if (!params_ok(prm) || batch <= 0 || batch > kMaxBatch || !workspace || !j_foot ||
      !foot_forces_grf || !joint_torques)
    return QLOCO_ERR_ARG;
  TorqueArgs a;
  a.prm = *prm;
  a.batch = batch;
  a.ws = (double *)workspace;
  a.j_foot = j_foot;
  a.grf = foot_forces_grf;
  a.tau = joint_torques;
  hipLaunchKernelGGL(a1_torque_kernel, dim3((unsigned)((4 * batch + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, a);
  QLOCO_HIP_CHECK(hipGetLastError(), "a1_torque_kernel launch");
  return QLOCO_OK;
}

extern "C" int qloco_a1_ctrl_get_state(int64_t batch, const void *workspace, double *state,
                                       void *stream) {
  if (batch <= 0 || batch > kMaxBatch || !workspace || !state) return QLOCO_ERR_ARG;
  const int64_t n = batch * REC;
  hipLaunchKernelGGL(a1_ctrl_copy_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, batch, (double *)workspace, state);
  QLOCO_HIP_CHECK(hipGetLastError(), "a1_ctrl_get_kernel launch");
  return QLOCO_OK;
}

extern "C" int qloco_a1_ctrl_set_state(int64_t batch, void *workspace, const double *state,
                                       void *stream) {
  if (batch <= 0 || batch > kMaxBatch || !workspace || !state) return QLOCO_ERR_ARG;
  const int64_t n = batch * REC;
  hipLaunchKernelGGL(a1_ctrl_copy_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, batch, (double *)workspace, (double *)state);
  QLOCO_HIP_CHECK(hipGetLastError(), "a1_ctrl_set_kernel launch");
  return QLOCO_OK;
}

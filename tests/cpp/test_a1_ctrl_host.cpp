// test_a1_ctrl_host.cpp -- qloco::A1RobotControlBatch (include/qloco.hpp)
// against the C ABI it stages for (qloco_a1_ctrl_*), on the same inputs: 24
// ticks (standstill, then a fast trot, torques past the hold-off) at B = 1 and
// B = 5, every output and the dense member state compared bit for bit -- the
// shim only stages.  Needs a GPU; no oracle link.  Prints ALL OK and exits 0.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "qloco.hpp"

static int fails = 0;
#define CHECK(c, ...)                                 \
  do {                                                \
    if (!(c)) {                                       \
      ++fails;                                        \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                       \
      std::printf("\n");                              \
    }                                                 \
  } while (0)
#define HIP_OK(e) CHECK((e) == hipSuccess, "%s", hipGetErrorString(e))

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uni(double lo, double hi) {  // splitmix64 -> [lo, hi)
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return lo + (hi - lo) * ((double)(z >> 11) / 9007199254740992.0);
}

static void fill(qloco::A1CtrlState &s, int tick) {
  s.movement_mode = tick < 4 ? 0 : 1;
  const double r = uni(-0.1, 0.1), p = uni(-0.1, 0.1), y = uni(-3.1, 3.1);
  const double cr = std::cos(r), sr = std::sin(r), cp = std::cos(p), sp = std::sin(p),
               cy = std::cos(y), sy = std::sin(y);
  const double R[9] = {cy * cp, sy * cp, -sp, cy * sp * sr - sy * cr, sy * sp * sr + cy * cr,
                       cp * sr, cy * sp * cr + sy * sr, sy * sp * cr - cy * sr, cp * cr};
  const double Rz[9] = {cy, sy, 0, -sy, cy, 0, 0, 0, 1};
  for (int k = 0; k < 9; ++k) s.root_rot_mat[k] = R[k], s.root_rot_mat_z[k] = Rz[k];
  for (int k = 0; k < 3; ++k) {
    s.root_pos[k] = uni(-0.5, 0.5) + (k == 2 ? 0.3 : 0.0);
    s.root_lin_vel[k] = uni(-0.4, 0.4);
    s.root_lin_vel_d[k] = k == 2 ? 0.0 : uni(-0.5, 0.5);
    s.root_euler_d[k] = uni(-0.1, 0.1);
  }
  const double feet[12] = {0.18, 0.13, -0.31, 0.18, -0.13, -0.31, -0.18, 0.13, -0.31, -0.18, -0.13, -0.31};
  for (int l = 0; l < 4; ++l) {
    double f[3];
    for (int k = 0; k < 3; ++k) f[k] = feet[3 * l + k] + uni(-0.03, 0.03);
    for (int k = 0; k < 3; ++k) s.foot_pos_abs[3 * l + k] = R[k] * f[0] + R[3 + k] * f[1] + R[6 + k] * f[2];
    s.foot_force[l] = uni(-5, 60);
    // a well-conditioned Jacobian: the stand pose's, perturbed
    const double J[9] = {0, 0.3, 0.08, -0.3, 0, 0, -0.15, 0, 0.14};
    for (int k = 0; k < 9; ++k) s.j_foot[9 * l + k] = J[k] + uni(-0.01, 0.01);
    s.foot_forces_grf[3 * l] = uni(-15, 15);
    s.foot_forces_grf[3 * l + 1] = uni(-15, 15);
    s.foot_forces_grf[3 * l + 2] = uni(0, 120);
  }
}

static void run(int B) {
  const double dt = 0.0025;
  qloco_a1_ctrl_params prm;
  qloco_a1_ctrl_params_default(&prm);
  for (int l = 0; l < 4; ++l) prm.gait_counter_speed[l] = 24;  // a 10-tick cycle
  qloco::A1RobotControlBatch ctl(B, &prm);
  const size_t n = B;
  void *ws = nullptr;
  double *d_in, *d_out, *d_rec;
  int32_t *d_mode;
  uint8_t *d_ct;
  HIP_OK(hipMalloc(&ws, (size_t)qloco_a1_ctrl_workspace_bytes(B)));
  HIP_OK(hipMalloc(&d_in, 8 * 95 * n));
  HIP_OK(hipMalloc(&d_out, 8 * 89 * n));
  HIP_OK(hipMalloc(&d_rec, 8 * QLOCO_A1_CTRL_STATE * n));
  HIP_OK(hipMalloc(&d_mode, 4 * n));
  HIP_OK(hipMalloc(&d_ct, 12 * n));
  if (fails) return;
  CHECK(qloco_a1_ctrl_reset(&prm, B, ws, nullptr) == QLOCO_OK, "reset");
  // field-major device staging of the direct calls
  double *i_dt = d_in, *i_pos = i_dt + n, *i_vel = i_pos + 3 * n, *i_vd = i_vel + 3 * n,
         *i_rot = i_vd + 3 * n, *i_rz = i_rot + 9 * n, *i_feet = i_rz + 9 * n, *i_ff = i_feet + 12 * n,
         *i_eul = i_ff + 4 * n, *i_J = i_eul + 3 * n, *i_grf = i_J + 36 * n;
  double *o_gc = d_out, *o_t = o_gc + 4 * n, *o_ang = o_t + 72 * n, *o_tau = o_ang + n;
  std::vector<qloco::A1CtrlState> st(n);
  std::memset(st.data(), 0, sizeof(qloco::A1CtrlState) * n);
  std::vector<double> in(95 * n), out(89 * n), rec(QLOCO_A1_CTRL_STATE * n), recs(QLOCO_A1_CTRL_STATE * n), eul(3 * n);
  std::vector<int32_t> mode(n);
  std::vector<uint8_t> ct(12 * n);
  bool swing_seen = false, torque_seen = false;
  for (int tick = 0; tick < 24; ++tick) {
    for (size_t b = 0; b < n; ++b) {
      fill(st[b], tick);
      mode[b] = st[b].movement_mode;
      in[b] = dt;
      std::memcpy(&in[n + 3 * b], st[b].root_pos, 24);
      std::memcpy(&in[4 * n + 3 * b], st[b].root_lin_vel, 24);
      std::memcpy(&in[7 * n + 3 * b], st[b].root_lin_vel_d, 24);
      std::memcpy(&in[10 * n + 9 * b], st[b].root_rot_mat, 72);
      std::memcpy(&in[19 * n + 9 * b], st[b].root_rot_mat_z, 72);
      std::memcpy(&in[28 * n + 12 * b], st[b].foot_pos_abs, 96);
      std::memcpy(&in[40 * n + 4 * b], st[b].foot_force, 32);
      std::memcpy(&in[44 * n + 3 * b], st[b].root_euler_d, 24);
      std::memcpy(&in[47 * n + 36 * b], st[b].j_foot, 288);
      std::memcpy(&in[83 * n + 12 * b], st[b].foot_forces_grf, 96);
    }
    HIP_OK(hipMemcpy(d_in, in.data(), 8 * 95 * n, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_mode, mode.data(), 4 * n, hipMemcpyHostToDevice));
    CHECK(qloco_a1_ctrl_plan_swing(&prm, B, ws, i_dt, d_mode, i_pos, i_vel, i_vd, i_rot, i_rz, i_feet,
                                   i_ff, d_ct, d_ct + 4 * n, d_ct + 8 * n, o_gc, o_t, o_t + 12 * n,
                                   o_t + 24 * n, o_t + 36 * n, o_t + 48 * n, o_t + 60 * n,
                                   nullptr) == QLOCO_OK, "plan_swing");
    CHECK(qloco_a1_ctrl_terrain(&prm, B, ws, i_pos, i_eul, o_ang, nullptr, nullptr) == QLOCO_OK, "terrain");
    CHECK(qloco_a1_ctrl_joint_torques(&prm, B, ws, i_J, i_grf, o_tau, nullptr) == QLOCO_OK, "torques");
    CHECK(qloco_a1_ctrl_get_state(B, ws, d_rec, nullptr) == QLOCO_OK, "get_state");
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out.data(), d_out, 8 * 89 * n, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(ct.data(), d_ct, 12 * n, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(eul.data(), i_eul, 24 * n, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(rec.data(), d_rec, 8 * QLOCO_A1_CTRL_STATE * n, hipMemcpyDeviceToHost));
    // the shim, called as GazeboA1ROS::main_update and the control thread do
    ctl.update_plan(st.data(), dt);
    ctl.generate_swing_legs_ctrl(st.data(), dt);
    for (size_t b = 0; b < n; ++b)
      for (int k = 0; k < 12; ++k) CHECK(st[b].joint_torques[k] == 0.0, "torques zeroed by the swing call");
    ctl.compute_terrain_pitch(st.data());
    ctl.compute_joint_torques(st.data());
    ctl.get_state(recs.data());
    for (size_t b = 0; b < n; ++b) {
      const qloco::A1CtrlState &s = st[b];
      CHECK(!std::memcmp(s.gait_counter, &out[4 * b], 32), "B=%d tick %d robot %zu gait_counter", B, tick, b);
      const double *f[6] = {s.foot_pos_target_rel, s.foot_pos_target_abs, s.foot_pos_target_world,
                            s.foot_pos_cur,        s.foot_forces_kin,     s.foot_pos_recent_contact};
      for (int q = 0; q < 6; ++q)
        CHECK(!std::memcmp(f[q], &out[(4 + 12 * q) * n + 12 * b], 96), "B=%d tick %d robot %zu field %d", B, tick, b, q);
      for (int l = 0; l < 4; ++l) {
        CHECK(s.contacts[l] == (ct[4 * b + l] != 0), "contacts");
        CHECK(s.plan_contacts[l] == (ct[4 * n + 4 * b + l] != 0), "plan_contacts");
        CHECK(s.early_contacts[l] == (ct[8 * n + 4 * b + l] != 0), "early_contacts");
        swing_seen |= !s.contacts[l];
      }
      CHECK(!std::memcmp(&s.terrain_pitch_angle, &out[76 * n + b], 8), "terrain_pitch_angle");
      CHECK(!std::memcmp(&s.root_euler_d[1], &eul[3 * b + 1], 8), "root_euler_d[1]");
      CHECK(!std::memcmp(s.joint_torques, &out[77 * n + 12 * b], 96), "B=%d tick %d robot %zu joint_torques", B, tick, b);
      for (int k = 0; k < 12; ++k) {
        CHECK(std::isfinite(s.joint_torques[k]), "finite torque");
        if (tick < 8) CHECK(s.joint_torques[k] == 0.0, "hold-off");
        torque_seen |= s.joint_torques[k] != 0.0;
      }
    }
    CHECK(!std::memcmp(rec.data(), recs.data(), 8 * QLOCO_A1_CTRL_STATE * n), "B=%d tick %d member state", B, tick);
  }
  CHECK(swing_seen && torque_seen, "the sequence reached swing legs and non-zero torques");
  bool thrown = false;
  try {
    ctl.generate_swing_legs_ctrl(st.data(), dt);  // without update_plan
  } catch (const qloco::Error &e) {
    thrown = e.status == QLOCO_ERR_ARG;
  }
  CHECK(thrown, "generate_swing_legs_ctrl without update_plan refused");
  for (void *p : {ws, (void *)d_in, (void *)d_out, (void *)d_rec, (void *)d_mode, (void *)d_ct})
    (void)hipFree(p);
  std::printf("A1RobotControlBatch B=%d: %s\n", B, fails ? "FAIL" : "ok");
}

int main() {
  try {
    bool thrown = false;
    try {
      qloco::A1RobotControlBatch bad(0);
    } catch (const qloco::Error &e) {
      thrown = e.status == QLOCO_ERR_ARG;
    }
    CHECK(thrown, "batch 0 refused");
    run(1);
    if (!fails) run(5);
  } catch (const std::exception &e) {
    std::printf("exception: %s\n", e.what());
    return 2;
  }
  if (fails) return 1;
  std::printf("ALL OK\n");
  return 0;
}

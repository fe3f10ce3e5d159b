// test_a1_est_host.cpp -- qloco::A1BasicEKFBatch (include/qloco.hpp) against
// the C ABI it stages for (qloco_a1_ekf_*), on the same inputs: init_state and
// three update_estimation ticks at B = 1 and B = 5, results (root_pos,
// root_lin_vel, estimated_contacts, x, P) compared bit for bit -- the shim
// only stages.  Needs a GPU; no oracle link.  Prints ALL OK and exits 0.
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

static void fill(qloco::A1EstState &s, int robot, int tick) {
  std::memset(&s, 0, sizeof(s));
  s.movement_mode = (robot % 3 == 0) ? 0 : 1;
  const double r = uni(-0.1, 0.1), p = uni(-0.1, 0.1), y = uni(-3.1, 3.1);
  const double cr = std::cos(r), sr = std::sin(r), cp = std::cos(p), sp = std::sin(p),
               cy = std::cos(y), sy = std::sin(y);
  const double R[9] = {cy * cp, sy * cp, -sp, cy * sp * sr - sy * cr, sy * sp * sr + cy * cr,
                       cp * sr, cy * sp * cr + sy * sr, sy * sp * cr - cy * sr, cp * cr};
  for (int k = 0; k < 9; ++k) s.root_rot_mat[k] = R[k];
  for (int k = 0; k < 3; ++k) {
    s.imu_acc[k] = uni(-0.5, 0.5) + (k == 2 ? 9.81 : 0.0);
    s.imu_ang_vel[k] = uni(-0.3, 0.3);
  }
  const double feet[12] = {0.18, 0.13, -0.31, 0.18, -0.13, -0.31, -0.18, 0.13, -0.31, -0.18, -0.13, -0.31};
  for (int k = 0; k < 12; ++k) {
    s.foot_pos_rel[k] = feet[k] + uni(-0.03, 0.03);
    s.foot_vel_rel[k] = uni(-0.5, 0.5);
  }
  for (int l = 0; l < 4; ++l) s.foot_force[l] = ((l + tick) % 2) ? uni(60, 140) : uni(-5, 20);
}

static void run(int B) {
  const double dt = 0.0025;
  qloco::A1BasicEKFBatch ekf(B);
  CHECK(!ekf.is_inited(), "is_inited before init_state");
  // direct C ABI on buffers of its own
  qloco_a1_ekf_params prm;
  qloco_a1_ekf_params_default(&prm);
  const size_t n = B;
  void *ws = nullptr;
  double *d_dt, *d_rot, *d_acc, *d_om, *d_fk, *d_fv, *d_ff, *d_pos, *d_vel, *d_x, *d_P;
  int32_t *d_mode;
  uint8_t *d_ct;
  HIP_OK(hipMalloc(&ws, (size_t)qloco_a1_ekf_workspace_bytes(B)));
  HIP_OK(hipMalloc(&d_dt, 8 * n));
  HIP_OK(hipMalloc(&d_rot, 8 * 9 * n));
  HIP_OK(hipMalloc(&d_acc, 8 * 3 * n));
  HIP_OK(hipMalloc(&d_om, 8 * 3 * n));
  HIP_OK(hipMalloc(&d_fk, 8 * 12 * n));
  HIP_OK(hipMalloc(&d_fv, 8 * 12 * n));
  HIP_OK(hipMalloc(&d_ff, 8 * 4 * n));
  HIP_OK(hipMalloc(&d_pos, 8 * 3 * n));
  HIP_OK(hipMalloc(&d_vel, 8 * 3 * n));
  HIP_OK(hipMalloc(&d_x, 8 * 18 * n));
  HIP_OK(hipMalloc(&d_P, 8 * 324 * n));
  HIP_OK(hipMalloc(&d_mode, 4 * n));
  HIP_OK(hipMalloc(&d_ct, 4 * n));
  if (fails) return;
  std::vector<qloco::A1EstState> st(n);
  std::vector<double> hdt(n, dt), rot(9 * n), acc(3 * n), om(3 * n), fk(12 * n), fv(12 * n),
      ff(4 * n), pos(3 * n), vel(3 * n), x(18 * n), P(324 * n), xs(18 * n), Ps(324 * n);
  std::vector<int32_t> mode(n);
  std::vector<uint8_t> ct(4 * n);
  for (int tick = 0; tick < 4; ++tick) {
    for (size_t b = 0; b < n; ++b) {
      fill(st[b], (int)b, tick);
      mode[b] = st[b].movement_mode;
      std::memcpy(&rot[9 * b], st[b].root_rot_mat, 72);
      std::memcpy(&acc[3 * b], st[b].imu_acc, 24);
      std::memcpy(&om[3 * b], st[b].imu_ang_vel, 24);
      std::memcpy(&fk[12 * b], st[b].foot_pos_rel, 96);
      std::memcpy(&fv[12 * b], st[b].foot_vel_rel, 96);
      std::memcpy(&ff[4 * b], st[b].foot_force, 32);
    }
    HIP_OK(hipMemcpy(d_dt, hdt.data(), 8 * n, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_mode, mode.data(), 4 * n, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_rot, rot.data(), 72 * n, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_acc, acc.data(), 24 * n, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_om, om.data(), 24 * n, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_fk, fk.data(), 96 * n, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_fv, fv.data(), 96 * n, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_ff, ff.data(), 32 * n, hipMemcpyHostToDevice));
    if (tick == 0) {  // GazeboA1ROS.cpp:205-209: the first tick only initialises
      ekf.init_state(st.data());
      CHECK(ekf.is_inited(), "is_inited after init_state");
      CHECK(qloco_a1_ekf_init(&prm, B, ws, d_rot, d_fk, nullptr) == QLOCO_OK, "ekf_init");
    } else {
      ekf.update_estimation(st.data(), dt);
      CHECK(qloco_a1_ekf_update(&prm, B, ws, d_dt, d_mode, d_rot, d_acc, d_om, d_fk, d_fv, d_ff,
                                d_pos, d_vel, d_ct, nullptr) == QLOCO_OK,
            "ekf_update");
      HIP_OK(hipDeviceSynchronize());
      HIP_OK(hipMemcpy(pos.data(), d_pos, 24 * n, hipMemcpyDeviceToHost));
      HIP_OK(hipMemcpy(vel.data(), d_vel, 24 * n, hipMemcpyDeviceToHost));
      HIP_OK(hipMemcpy(ct.data(), d_ct, 4 * n, hipMemcpyDeviceToHost));
      for (size_t b = 0; b < n; ++b) {
        CHECK(!std::memcmp(st[b].root_pos, &pos[3 * b], 24), "B=%d tick %d robot %zu root_pos", B, tick, b);
        CHECK(!std::memcmp(st[b].root_lin_vel, &vel[3 * b], 24), "B=%d tick %d robot %zu root_lin_vel", B, tick, b);
        CHECK(!std::memcmp(st[b].estimated_root_pos, &pos[3 * b], 24), "estimated_root_pos");
        CHECK(!std::memcmp(st[b].estimated_root_vel, &vel[3 * b], 24), "estimated_root_vel");
        for (int l = 0; l < 4; ++l)
          CHECK(st[b].estimated_contacts[l] == (ct[4 * b + l] != 0), "contacts robot %zu leg %d", b, l);
        for (int k = 0; k < 3; ++k) CHECK(std::isfinite(pos[3 * b + k]), "finite root_pos");
      }
    }
    CHECK(qloco_a1_ekf_get_state(B, ws, d_x, d_P, nullptr) == QLOCO_OK, "get_state");
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(x.data(), d_x, 8 * 18 * n, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(P.data(), d_P, 8 * 324 * n, hipMemcpyDeviceToHost));
    ekf.get_state(xs.data(), Ps.data());
    CHECK(!std::memcmp(x.data(), xs.data(), 8 * 18 * n), "B=%d tick %d x", B, tick);
    CHECK(!std::memcmp(P.data(), Ps.data(), 8 * 324 * n), "B=%d tick %d P", B, tick);
    if (tick == 0) CHECK(P[0] == 3.0 && P[1] == 0.0 && x[2] == 0.09, "init_state values");
  }
  for (void *p : {ws, (void *)d_dt, (void *)d_rot, (void *)d_acc, (void *)d_om, (void *)d_fk,
                  (void *)d_fv, (void *)d_ff, (void *)d_pos, (void *)d_vel, (void *)d_x, (void *)d_P,
                  (void *)d_mode, (void *)d_ct})
    (void)hipFree(p);
  std::printf("A1BasicEKFBatch B=%d: %s\n", B, fails ? "FAIL" : "ok");
}

int main() {
  try {
    bool thrown = false;
    try {
      qloco::A1BasicEKFBatch bad(0);
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

// test_a1qp_body_host -- qloco::A1QpBatch::set_bodies (include/qloco.hpp):
// eight robots with four bodies (row b % 4) in one object against eight
// one-robot objects whose params carry the row's values -- forces, status and
// iterations equal exactly --, a refused row (QLOCO_ERR_ARG and NaN forces for
// that robot alone), and set_bodies(nullptr) back to params' result.  Run by
// tests/test_a1qp_body_gpu.py; prints "ALL OK".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "qloco.hpp"

static int fails = 0;
#define CHECK(c, ...)            \
  do {                           \
    if (!(c)) {                  \
      std::printf("FAIL: ");     \
      std::printf(__VA_ARGS__);  \
      std::printf("\n");         \
      ++fails;                   \
    }                            \
  } while (0)

static qloco_a1_body body(const qloco_a1_params &p, int k) {
  qloco_a1_body r;
  CHECK(qloco_a1_body_from_params(&p, 1, &r) == QLOCO_OK, "qloco_a1_body_from_params");
  switch (k) {
    case 1: r.robot_mass = 30.0, r.f_max = 60.0; break;
    case 2: r.mu = 0.2, r.f_min = 20.0; break;
    case 3: r.kp_linear[2] = 1500.0, r.kd_angular[0] = 9.0, r.q_diag[3] = 100.0, r.r = 1e-2; break;
    default: break;  // params' body
  }
  return r;
}

// params with the row's values: the layouts agree field by field
static qloco_a1_params with_body(qloco_a1_params p, const qloco_a1_body &r) {
  for (int k = 0; k < 3; ++k) {
    p.kp_linear[k] = r.kp_linear[k];
    p.kd_linear[k] = r.kd_linear[k];
    p.kp_angular[k] = r.kp_angular[k];
    p.kd_angular[k] = r.kd_angular[k];
  }
  p.robot_mass = r.robot_mass;
  for (int k = 0; k < 6; ++k) p.q_diag[k] = r.q_diag[k];
  p.r = r.r, p.mu = r.mu, p.f_min = r.f_min, p.f_max = r.f_max;
  return p;
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

int main() {
  try {
    const int B = 8;
    std::vector<qloco::A1QpState> st(B);
    for (int b = 0; b < B; ++b) {
      qloco::A1QpState &s = st[b];
      s = qloco::A1QpState{};
      const double yaw = 0.4 * b - 1.3;
      const double c = std::cos(yaw), sn = std::sin(yaw);
      const double R[9] = {c, sn, 0, -sn, c, 0, 0, 0, 1};
      for (int k = 0; k < 9; ++k) s.root_rot_mat[k] = s.root_rot_mat_z[k] = R[k];
      s.root_euler[2] = yaw;
      s.root_euler_d[2] = yaw + 0.05 * (b - 3);
      s.root_lin_vel[0] = 0.05 * b, s.root_lin_vel[1] = -0.03 * b;
      s.root_lin_vel_d[0] = 0.3;
      s.root_ang_vel[2] = 0.1 * (b - 4);
      s.root_pos[2] = 0.28;
      s.root_pos_d[2] = 0.30;
      const double fb[12] = {0.17, 0.15, -0.3, 0.17, -0.15, -0.3, -0.17, 0.15, -0.3, -0.17, -0.15, -0.3};
      for (int l = 0; l < 4; ++l)  // foot_pos_abs = R * foot_pos_rel
        for (int r = 0; r < 3; ++r)
          s.foot_pos_abs[3 * l + r] = R[r] * fb[3 * l] + R[3 + r] * fb[3 * l + 1] + R[6 + r] * fb[3 * l + 2];
      for (int l = 0; l < 4; ++l) s.contacts[l] = (b & 1) ? (l == 1 || l == 2) : (l == 0 || l == 3);
      if (b == 5) s.contacts[0] = s.contacts[1] = s.contacts[2] = s.contacts[3] = true;
    }
    qloco::A1QpBatch fleet(B);
    const qloco_a1_params base = fleet.params;
    std::vector<qloco_a1_body> rows(B);
    for (int b = 0; b < B; ++b) rows[b] = body(base, b % 4);

    // params' body for everyone, before any rows
    std::vector<double> f_prm(B * 12, 0.0);
    fleet.compute_grf(st.data(), f_prm.data());
    const std::vector<int32_t> it_prm = fleet.iters;

    // one-robot objects: the row's values in the params
    std::vector<double> want(B * 12, 0.0);
    std::vector<int32_t> want_it(B), want_st(B);
    for (int b = 0; b < B; ++b) {
      const qloco_a1_params p = with_body(base, rows[b]);
      qloco::A1QpBatch one(1, &p);
      one.compute_grf(&st[b], &want[b * 12]);
      want_it[b] = one.iters[0];
      want_st[b] = one.status[0];
    }

    fleet.set_bodies(rows.data());
    std::vector<double> got(B * 12, 0.0);
    fleet.compute_grf(st.data(), got.data());
    int differ = 0, solved = 0;
    for (int b = 0; b < B; ++b) {
      CHECK(fleet.status[b] == want_st[b], "robot %d status %d / %d", b, fleet.status[b], want_st[b]);
      solved += fleet.status[b] == QLOCO_OK;
      CHECK(fleet.iters[b] == want_it[b], "robot %d iters %d vs %d", b, fleet.iters[b], want_it[b]);
      for (int k = 0; k < 12; ++k) {
        CHECK(same_bits(got[b * 12 + k], want[b * 12 + k]), "robot %d force %d: %.17g vs %.17g", b, k,
              got[b * 12 + k], want[b * 12 + k]);
        if (b % 4) differ += !same_bits(got[b * 12 + k], f_prm[b * 12 + k]);
      }
    }
    CHECK(differ > 0, "the rows changed no force of any robot with another body");
    CHECK(solved >= B / 2, "only %d of %d robots solved", solved, B);

    // an invalid row: that robot alone is refused
    std::vector<qloco_a1_body> bad = rows;
    bad[3].robot_mass = 0.0;
    CHECK(qloco_a1_body_check(&bad[3]) == QLOCO_ERR_ARG && qloco_a1_body_check(&rows[3]) == QLOCO_OK,
          "qloco_a1_body_check");
    fleet.set_bodies(bad.data());
    std::vector<double> gb(B * 12, -7.0);
    fleet.compute_grf(st.data(), gb.data());
    for (int b = 0; b < B; ++b) {
      CHECK(fleet.status[b] == (b == 3 ? QLOCO_ERR_ARG : want_st[b]), "invalid row: robot %d status %d", b,
            fleet.status[b]);
      CHECK(fleet.iters[b] == (b == 3 ? 0 : want_it[b]), "invalid row: robot %d iters %d", b, fleet.iters[b]);
      for (int k = 0; k < 12; ++k)
        CHECK(b == 3 ? std::isnan(gb[b * 12 + k]) : same_bits(gb[b * 12 + k], want[b * 12 + k]),
              "invalid row: robot %d force %d", b, k);
    }

    // back to params' body
    fleet.set_bodies(nullptr);
    std::vector<double> again(B * 12, 0.0);
    fleet.compute_grf(st.data(), again.data());
    for (int b = 0; b < B; ++b) {
      CHECK(fleet.iters[b] == it_prm[b], "nullptr: robot %d iters %d vs %d", b, fleet.iters[b], it_prm[b]);
      for (int k = 0; k < 12; ++k)
        CHECK(same_bits(again[b * 12 + k], f_prm[b * 12 + k]), "nullptr: robot %d force %d", b, k);
    }
    if (fails) {
      std::printf("%d check(s) failed\n", fails);
      return 1;
    }
    std::printf("ALL OK\n");
    return 0;
  } catch (const std::exception &e) {
    std::printf("exception: %s\n", e.what());
    return 1;
  }
}

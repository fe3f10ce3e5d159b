// test_srbd_model_host -- qloco::ConvexMpcBatch::set_models (include/qloco.hpp):
// eight robots with the five bodies of tests/test_srbd_model_gpu.py (row
// b % 5) in one object against eight one-robot objects whose spec carries
// the row's values -- forces, status and iterations equal exactly, on the
// first call and on the persistent solver's update path -- and
// set_models(nullptr) back to the spec's result.  Run by
// tests/test_srbd_model_gpu.py; prints "ALL OK".
#include <cmath>
#include <cstdio>
#include <cstdlib>
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

static qloco_srbd_model body(const qloco_srbd_spec &sp, int k) {
  qloco_srbd_model m;
  CHECK(qloco_srbd_model_from_spec(&sp, 1, &m) == QLOCO_OK, "qloco_srbd_model_from_spec");
  auto diag = [&](float xx, float yy, float zz) {
    for (int i = 0; i < 9; ++i) m.inertia[i] = 0.0f;
    m.inertia[0] = xx, m.inertia[4] = yy, m.inertia[8] = zz;
  };
  auto scale = [&](float s) {
    for (int i = 0; i < 9; ++i) m.inertia[i] = s * sp.inertia[i];
  };
  switch (k) {
    case 1: m.mass = 12.0f, diag(0.0158533f, 0.0377999f, 0.0456542f), m.mu = 0.3f, m.fz_min = 0.f, m.fz_max = 180.f; break;
    case 2: m.mass = 13.5f, diag(0.0178533f, 0.0377999f, 0.0456542f), m.mu = 0.3f, m.fz_min = 0.f, m.fz_max = 180.f; break;
    case 3: m.mass = 9.0f, scale(0.8f), m.mu = 0.6f, m.fz_min = 0.f, m.fz_max = 120.f; break;
    case 4: m.mass = 18.0f, scale(1.5f), m.mu = 0.2f, m.fz_min = 0.f, m.fz_max = 250.f; break;
    default: break;  // the spec's body
  }
  return m;
}

int main() {
  try {
    const int B = 8;
    std::vector<qloco::A1MpcState> st(B);
    for (int b = 0; b < B; ++b) {
      auto &s = st[b];
      s = qloco::A1MpcState{};
      s.root_pos[2] = 0.30;
      s.root_pos_d[2] = 0.30;
      s.root_euler[2] = 0.1 * b;
      s.root_lin_vel[0] = 0.05 * b;
      s.root_lin_vel_d[0] = 0.3;
      const double c = std::cos(0.1 * b), sn = std::sin(0.1 * b);
      const double R[9] = {c, sn, 0, -sn, c, 0, 0, 0, 1};
      for (int k = 0; k < 9; ++k) s.root_rot_mat[k] = R[k];
      const double feet[12] = {0.15, 0.127, -0.31, 0.15, -0.127, -0.31,
                               -0.225, 0.127, -0.31, -0.225, -0.127, -0.31};
      for (int k = 0; k < 12; ++k) s.foot_pos_abs[k] = feet[k];
      const bool ph = b & 1;
      s.contacts[0] = s.contacts[3] = ph;
      s.contacts[1] = s.contacts[2] = !ph;
    }
    qloco::ConvexMpcBatch fleet(B);
    const qloco_srbd_spec base = fleet.spec;
    std::vector<qloco_srbd_model> rows(B);
    for (int b = 0; b < B; ++b) rows[b] = body(base, b % 5);

    // the spec's body for everyone, before any rows
    std::vector<double> f_spec(B * 12, 0.0);
    fleet.compute_grf(st.data(), f_spec.data());
    std::vector<int32_t> it_spec = fleet.iters;

    // one-robot objects: the row's values in the spec
    std::vector<double> want(2 * B * 12, 0.0);
    std::vector<int32_t> want_it(2 * B), want_st(2 * B);
    for (int b = 0; b < B; ++b) {
      qloco_srbd_spec sp = base;
      sp.mass = rows[b].mass;
      for (int i = 0; i < 9; ++i) sp.inertia[i] = rows[b].inertia[i];
      sp.mu = rows[b].mu, sp.fz_min = rows[b].fz_min, sp.fz_max = rows[b].fz_max;
      sp.warm_start = 2, sp.literal_full_qp = 1;
      qloco::ConvexMpcBatch one(1, &sp);
      for (int call = 0; call < 2; ++call) {
        one.compute_grf(&st[b], &want[(call * B + b) * 12]);
        want_it[call * B + b] = one.iters[0];
        want_st[call * B + b] = one.status[0];
      }
    }

    fleet.reset();
    fleet.set_models(rows.data());
    int differ = 0;
    for (int call = 0; call < 2; ++call) {
      std::vector<double> got(B * 12, 0.0);
      fleet.compute_grf(st.data(), got.data());
      for (int b = 0; b < B; ++b) {
        CHECK(fleet.status[b] == QLOCO_OK && want_st[call * B + b] == QLOCO_OK, "call %d robot %d status %d / %d",
              call, b, fleet.status[b], want_st[call * B + b]);
        CHECK(fleet.iters[b] == want_it[call * B + b], "call %d robot %d iters %d vs %d", call, b, fleet.iters[b],
              want_it[call * B + b]);
        for (int k = 0; k < 12; ++k)
          CHECK(got[b * 12 + k] == want[(call * B + b) * 12 + k], "call %d robot %d force %d: %.9g vs %.9g", call, b,
                k, got[b * 12 + k], want[(call * B + b) * 12 + k]);
        if (call == 0 && b % 5)
          for (int k = 0; k < 12; ++k) differ += got[b * 12 + k] != f_spec[b * 12 + k];
      }
    }
    CHECK(differ > 0, "the rows changed no force of any robot with another body");

    // an invalid row: that robot alone is refused and keeps its forces
    std::vector<qloco_srbd_model> bad = rows;
    bad[3].mass = 0.0f;
    fleet.reset();
    fleet.set_models(bad.data());
    std::vector<double> got(B * 12, -7.0);
    fleet.compute_grf(st.data(), got.data());
    for (int b = 0; b < B; ++b) {
      CHECK(fleet.status[b] == (b == 3 ? QLOCO_ERR_ARG : QLOCO_OK), "invalid row: robot %d status %d", b,
            fleet.status[b]);
      for (int k = 0; k < 12; ++k)
        CHECK(got[b * 12 + k] == (b == 3 ? -7.0 : want[b * 12 + k]), "invalid row: robot %d force %d", b, k);
    }

    // back to the spec's body
    fleet.reset();
    fleet.set_models(nullptr);
    std::vector<double> again(B * 12, 0.0);
    fleet.compute_grf(st.data(), again.data());
    for (int b = 0; b < B; ++b) {
      CHECK(fleet.iters[b] == it_spec[b], "nullptr: robot %d iters %d vs %d", b, fleet.iters[b], it_spec[b]);
      for (int k = 0; k < 12; ++k)
        CHECK(again[b * 12 + k] == f_spec[b * 12 + k], "nullptr: robot %d force %d", b, k);
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

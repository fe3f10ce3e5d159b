// test_force_body_host -- set_bodies of qloco::Dynamiccclass, ServoForceBlock
// and Go1ServoBatch (include/qloco.hpp): eight robots with four bodies (row
// b % 4) in one object against eight one-robot objects -- for Dynamiccclass
// with the row's values in their params, for the two servo classes (whose
// params cannot carry a mass) with the robot's row alone -- every result member
// equal bit for bit; a refused row (QLOCO_ERR_ARG for that robot alone, its
// members kept / its outputs NaN); set_bodies(nullptr) back to the params'
// result.  Run by tests/test_force_body_gpu.py; prints "ALL OK".
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

static const int B = 8;

static qloco_force_body body(const qloco_force_params &p, int k) {
  qloco_force_body r;
  CHECK(qloco_force_body_from_params(&p, 1, &r) == QLOCO_OK, "qloco_force_body_from_params");
  switch (k) {
    case 1: r.mass = 14.0, r.mu = 0.5; break;
    case 2: r.mass = 17.5, r.fz_max = 90.0, r.momentum[0] *= 1.5, r.momentum[4] *= 1.25; break;
    case 3: r.alpha = 2000.0, r.beta = 300.0, r.gamma = 50.0, r.mu = 0.15, r.momentum[8] *= 0.5; break;
    default: break;  // params' body
  }
  return r;
}

static bool same(const double *a, const double *b, size_t n) { return std::memcmp(a, b, n * sizeof(double)) == 0; }
static bool all_nan(const double *a, size_t n) {
  for (size_t k = 0; k < n; ++k)
    if (!std::isnan(a[k])) return false;
  return true;
}
static bool all_finite(const double *a, size_t n) {
  for (size_t k = 0; k < n; ++k)
    if (!std::isfinite(a[k])) return false;
  return true;
}

// ---- Dynamiccclass: two ticks of force_distribution + force_opt
struct DynIn {
  double com[3], leg[12], F[6], rf[3], lf[3], FT[6], y;
  int mode, rs;
};
static DynIn dyn_in(int b, int tick) {
  DynIn s;
  const double ph = 0.37 * b + 0.11 * tick;
  const double body[3] = {0.01 * std::sin(ph), 0.02 * std::cos(ph), 0.30};
  const double home[12] = {0.150786, -0.12675, 0, 0.150786, 0.12675, 0, -0.225414, -0.12675, 0, -0.225414, 0.12675, 0};
  for (int k = 0; k < 3; ++k) s.com[k] = body[k];
  for (int k = 0; k < 12; ++k) s.leg[k] = home[k] + (k % 3 < 2 ? body[k % 3] : 0.0);
  for (int k = 0; k < 3; ++k) {
    s.rf[k] = (s.leg[k] + s.leg[9 + k]) / 2;
    s.lf[k] = (s.leg[3 + k] + s.leg[6 + k]) / 2;
  }
  s.mode = b % 3 == 0 ? 101 : b % 3 == 1 ? 102 : 103;
  s.rs = (b + tick) % 3;
  s.y = s.mode == 101 ? 0.75 : s.mode == 102 ? 0.0 : 0.11;
  const double Fs[6] = {4.0 * std::sin(ph), -3.0 * std::cos(ph), 117.6 + 5.0 * std::sin(2 * ph),
                        0.02 * std::sin(ph), -0.03 * std::cos(ph), 0.01};
  for (int k = 0; k < 6; ++k) s.FT[k] = Fs[k];
  for (int k = 0; k < 3; ++k) {
    s.F[k] = s.rs == 0 ? Fs[k] : s.rs == 1 ? 0.0 : 0.45 * Fs[k];
    s.F[3 + k] = Fs[k] - s.F[k];
  }
  return s;
}
static void dyn_tick(qloco::Dynamiccclass &d, int first, int tick) {
  for (int r = 0; r < d.batch(); ++r) {
    const DynIn s = dyn_in(first + r, tick);
    d.force_distribution(s.com, s.leg, s.F, s.mode, s.y, s.rf, s.lf, r);
    d.force_opt(s.com, s.leg, s.leg + 3, s.leg + 6, s.leg + 9, s.FT, s.mode, s.rs, s.y, r);
  }
}

static void test_dynamiccclass(const std::vector<qloco_force_body> &rows) {
  qloco_force_params base;
  qloco_force_params_default(&base);
  qloco::Dynamiccclass fleet(B, &base), plain(B, &base);
  fleet.set_bodies(rows.data());
  std::vector<qloco::Dynamiccclass *> one;
  for (int b = 0; b < B; ++b) {
    const qloco_force_body &r = rows[b];
    const qloco_force_params p = {r.mass, r.alpha, r.beta, r.gamma, r.fz_max, r.mu};
    one.push_back(new qloco::Dynamiccclass(1, &p));
  }
  int differ = 0;
  for (int tick = 0; tick < 2; ++tick) {
    dyn_tick(fleet, 0, tick);
    dyn_tick(plain, 0, tick);
    for (int b = 0; b < B; ++b) {
      dyn_tick(*one[b], b, tick);
      CHECK(fleet.status[b] == one[b]->status[0] && fleet.iters[b] == one[b]->iters[0] &&
                fleet.qp_solution[b] == one[b]->qp_solution[0],
            "Dynamiccclass tick %d robot %d: status %d / %d, iters %d / %d", tick, b, fleet.status[b],
            one[b]->status[0], fleet.iters[b], one[b]->iters[0]);
      CHECK(same(&fleet.grf_opt[12 * b], one[b]->grf_opt.data(), 12), "Dynamiccclass tick %d robot %d grf_opt", tick, b);
      CHECK(same(&fleet.F_leg_ref[12 * b], one[b]->F_leg_ref.data(), 12), "Dynamiccclass tick %d robot %d F_leg_ref", tick, b);
      CHECK(same(&fleet.F_leg_guess[12 * b], one[b]->F_leg_guess.data(), 12), "Dynamiccclass tick %d robot %d F_leg_guess", tick, b);
      if (b % 4 == 1 || b % 4 == 3) differ += !same(&fleet.grf_opt[12 * b], &plain.grf_opt[12 * b], 12);
    }
  }
  CHECK(differ > 0, "Dynamiccclass: the rows changed no grf_opt");
  // a refused row: that robot's members stay, everyone else goes on
  std::vector<qloco_force_body> bad = rows;
  bad[3].mass = 0.0;
  CHECK(qloco_force_body_check(&bad[3]) == QLOCO_ERR_ARG && qloco_force_body_check(&rows[3]) == QLOCO_OK,
        "qloco_force_body_check");
  const std::vector<double> grf_before = fleet.grf_opt, ref_before = fleet.F_leg_ref;
  fleet.set_bodies(bad.data());
  dyn_tick(fleet, 0, 2);
  for (int b = 0; b < B; ++b) {
    dyn_tick(*one[b], b, 2);
    if (b == 3) {
      CHECK(fleet.status[b] == QLOCO_ERR_ARG && fleet.qp_solution[b] == 0 && fleet.iters[b] == 0,
            "Dynamiccclass refused robot: status %d", fleet.status[b]);
      CHECK(same(&fleet.grf_opt[12 * b], &grf_before[12 * b], 12) && same(&fleet.F_leg_ref[12 * b], &ref_before[12 * b], 12),
            "Dynamiccclass refused robot: members moved");
      CHECK(all_nan(&fleet.F_leg_guess[12 * b], 12), "Dynamiccclass refused robot: F_leg_guess");
    } else {
      CHECK(fleet.status[b] == one[b]->status[0] && same(&fleet.grf_opt[12 * b], one[b]->grf_opt.data(), 12),
            "Dynamiccclass beside a refused robot: robot %d", b);
    }
  }
  // nullptr: the params again (a fresh pair, so that both carry the same members)
  qloco::Dynamiccclass back(B, &base), ref(B, &base);
  back.set_bodies(rows.data());
  back.set_bodies(nullptr);
  dyn_tick(back, 0, 0);
  dyn_tick(ref, 0, 0);
  CHECK(same(back.grf_opt.data(), ref.grf_opt.data(), 12 * B) && back.iters == ref.iters, "Dynamiccclass set_bodies(nullptr)");
  for (auto *p : one) delete p;
}

// ---- ServoForceBlock: three ticks
struct BlockIn {
  double coma[3], com[3], rf[3], lf[3], bp[3], foot[12], y, J[36], rm[12], ve[12];
  int32_t rs, mode, cnt;
};
static BlockIn block_in(int b, int tick) {
  BlockIn s;
  const DynIn d = dyn_in(b, tick);
  const double ph = 0.37 * b + 0.11 * tick;
  for (int k = 0; k < 3; ++k) {
    s.coma[k] = 0.4 * std::sin(ph + k);
    s.com[k] = d.com[k] + 0.002 * std::cos(ph + k);
    s.rf[k] = d.rf[k], s.lf[k] = d.lf[k], s.bp[k] = d.com[k];
  }
  for (int k = 0; k < 12; ++k) {
    s.foot[k] = d.leg[k];
    s.rm[k] = d.leg[k] - d.com[k % 3] + 0.001 * std::sin(ph + k);
    s.ve[k] = 0.05 * std::cos(ph + k);
  }
  for (int l = 0; l < 4; ++l)
    for (int k = 0; k < 9; ++k) s.J[9 * l + k] = (k % 4 == 0 ? 0.3 : 0.0) + 0.1 * std::sin(ph + l + 0.7 * k);
  s.y = d.y, s.rs = d.rs, s.mode = d.mode, s.cnt = tick;
  return s;
}
static void block_tick(qloco::ServoForceBlock &blk, int first, int tick) {
  const int n = blk.batch();
  std::vector<double> coma(3 * n), com(3 * n), rf(3 * n), lf(3 * n), bp(3 * n), foot(12 * n), y(n), J(36 * n),
      rm(12 * n), ve(12 * n);
  std::vector<int32_t> rs(n), mode(n), cnt(n);
  for (int r = 0; r < n; ++r) {
    const BlockIn s = block_in(first + r, tick);
    std::memcpy(&coma[3 * r], s.coma, sizeof(s.coma));
    std::memcpy(&com[3 * r], s.com, sizeof(s.com));
    std::memcpy(&rf[3 * r], s.rf, sizeof(s.rf));
    std::memcpy(&lf[3 * r], s.lf, sizeof(s.lf));
    std::memcpy(&bp[3 * r], s.bp, sizeof(s.bp));
    std::memcpy(&foot[12 * r], s.foot, sizeof(s.foot));
    std::memcpy(&J[36 * r], s.J, sizeof(s.J));
    std::memcpy(&rm[12 * r], s.rm, sizeof(s.rm));
    std::memcpy(&ve[12 * r], s.ve, sizeof(s.ve));
    y[r] = s.y, rs[r] = s.rs, mode[r] = s.mode, cnt[r] = s.cnt;
  }
  blk.step(coma.data(), com.data(), rf.data(), lf.data(), bp.data(), foot.data(), rs.data(), mode.data(), y.data(),
           cnt.data(), J.data(), rm.data(), ve.data());
}

static void test_block(const std::vector<qloco_force_body> &rows) {
  qloco::ServoForceBlock fleet(B), plain(B), back(B);
  fleet.set_bodies(rows.data());
  back.set_bodies(rows.data());
  back.set_bodies(nullptr);
  std::vector<qloco::ServoForceBlock *> one;
  for (int b = 0; b < B; ++b) {
    one.push_back(new qloco::ServoForceBlock(1));
    one[b]->set_bodies(&rows[b]);
  }
  std::vector<qloco_force_body> bad = rows;
  bad[5].mu = -0.1;
  int differ = 0;
  for (int tick = 0; tick < 3; ++tick) {
    const bool refuse = tick == 2;
    if (refuse) fleet.set_bodies(bad.data());
    block_tick(fleet, 0, tick);
    block_tick(plain, 0, tick);
    block_tick(back, 0, tick);
    for (int b = 0; b < B; ++b) {
      block_tick(*one[b], b, tick);
      if (refuse && b == 5) {
        CHECK(fleet.status[b] == QLOCO_ERR_ARG && fleet.qp_solution[b] == 0, "block refused robot: status %d", fleet.status[b]);
        CHECK(all_nan(&fleet.grf_opt[12 * b], 12) && all_nan(&fleet.Legs_torque[12 * b], 12), "block refused robot: outputs");
        continue;
      }
      CHECK(fleet.status[b] == one[b]->status[0], "block tick %d robot %d status %d / %d", tick, b, fleet.status[b], one[b]->status[0]);
      CHECK(same(&fleet.F_sum[6 * b], one[b]->F_sum.data(), 6) && same(&fleet.Force_L_R[6 * b], one[b]->Force_L_R.data(), 6),
            "block tick %d robot %d F_sum / Force_L_R", tick, b);
      CHECK(same(&fleet.grf_opt[12 * b], one[b]->grf_opt.data(), 12), "block tick %d robot %d grf_opt", tick, b);
      CHECK(same(&fleet.Legs_torque[12 * b], one[b]->Legs_torque.data(), 12), "block tick %d robot %d Legs_torque", tick, b);
      if (b % 4 == 0)
        CHECK(same(&fleet.grf_opt[12 * b], &plain.grf_opt[12 * b], 12) && same(&fleet.F_sum[6 * b], &plain.F_sum[6 * b], 6),
              "block tick %d robot %d: the params' row is not the params", tick, b);
      else
        differ += !same(&fleet.F_sum[6 * b], &plain.F_sum[6 * b], 6) || !same(&fleet.grf_opt[12 * b], &plain.grf_opt[12 * b], 12);
    }
    CHECK(same(back.grf_opt.data(), plain.grf_opt.data(), 12 * B) && same(back.Legs_torque.data(), plain.Legs_torque.data(), 12 * B) &&
              same(back.F_sum.data(), plain.F_sum.data(), 6 * B),
          "block tick %d set_bodies(nullptr)", tick);
  }
  CHECK(differ > 0, "block: the rows changed nothing");
  for (auto *p : one) delete p;
}

// ---- Go1ServoBatch: two stand-up ticks, then three of the gait branch
static void go1_tick(qloco::Go1ServoBatch &s, int first, int tick) {
  const int n = s.batch();
  std::vector<double> q(12 * n), quat(4 * n), gait(100 * n, 0.0), y(n);
  std::vector<int32_t> mode(n);
  for (int r = 0; r < n; ++r) {
    const int b = first + r;
    const double ph = 0.37 * b + 0.05 * tick;
    const double tgt[3] = {0.0, 0.87, -1.5};
    for (int k = 0; k < 12; ++k) q[12 * r + k] = tgt[k % 3] + 0.05 * std::sin(ph + k);
    const double roll = 0.1 * std::sin(ph), w = std::cos(roll / 2);
    quat[4 * r] = w, quat[4 * r + 1] = std::sin(roll / 2), quat[4 * r + 2] = 0.0, quat[4 * r + 3] = 0.0;
    double *g = &gait[100 * r];
    g[0] = 0.002 * std::sin(ph), g[1] = 0.002 * std::cos(ph), g[2] = 0.29;
    g[9] = 0.01, g[10] = -0.12675, g[11] = 0.0;
    g[6] = -0.01, g[7] = 0.12675, g[8] = 0.0;
    for (int k = 0; k < 3; ++k) g[39 + k] = 1.5 * std::sin(ph + k), g[73 + k] = 0.5 * std::cos(ph + k);
    g[99] = (b + tick) % 3;
    mode[r] = b % 3 == 0 ? 101 : b % 3 == 1 ? 102 : 103;
    y[r] = mode[r] == 101 ? 0.75 : mode[r] == 102 ? 0.0 : 0.11;
  }
  s.tick(q.data(), quat.data(), gait.data(), mode.data(), y.data());
}

static void test_go1(const std::vector<qloco_force_body> &rows) {
  qloco_go1_servo_params prm;
  qloco_go1_servo_params_default(&prm);
  prm.stand_duration = 0.0015;  // ticks 0 and 1 stand up
  qloco::Go1ServoBatch fleet(B, &prm), plain(B, &prm), back(B, &prm);
  std::vector<qloco_force_body> bad = rows;
  bad[6].fz_max = INFINITY;
  fleet.set_bodies(bad.data());  // while standing up no row is read: nothing is refused
  back.set_bodies(rows.data());
  back.set_bodies(nullptr);
  std::vector<qloco::Go1ServoBatch *> one;
  for (int b = 0; b < B; ++b) {
    one.push_back(new qloco::Go1ServoBatch(1, &prm));
    one[b]->set_bodies(&rows[b]);
  }
  int differ = 0;
  for (int tick = 0; tick < 5; ++tick) {
    if (tick == 2) fleet.set_bodies(rows.data());
    if (tick == 4) fleet.set_bodies(bad.data());
    go1_tick(fleet, 0, tick);
    go1_tick(plain, 0, tick);
    go1_tick(back, 0, tick);
    for (int b = 0; b < B; ++b) {
      go1_tick(*one[b], b, tick);
      if (tick == 4 && b == 6) {
        CHECK(all_nan(&fleet.grf_opt[12 * b], 12) && all_nan(&fleet.Legs_torque[12 * b], 12), "go1 refused robot: outputs");
        CHECK(same(&fleet.q_cmd[12 * b], one[b]->q_cmd.data(), 12), "go1 refused robot: q_cmd");
        continue;
      }
      CHECK(same(&fleet.grf_opt[12 * b], one[b]->grf_opt.data(), 12), "go1 tick %d robot %d grf_opt", tick, b);
      CHECK(same(&fleet.Legs_torque[12 * b], one[b]->Legs_torque.data(), 12), "go1 tick %d robot %d Legs_torque", tick, b);
      CHECK(same(&fleet.q_cmd[12 * b], one[b]->q_cmd.data(), 12), "go1 tick %d robot %d q_cmd", tick, b);
      CHECK(same(&fleet.joint2simulation[100 * b], one[b]->joint2simulation.data(), 100), "go1 tick %d robot %d joint2simulation", tick, b);
      if (tick >= 2 && b % 4) differ += !same(&fleet.grf_opt[12 * b], &plain.grf_opt[12 * b], 12);
    }
    CHECK(same(back.grf_opt.data(), plain.grf_opt.data(), 12 * B) && same(back.Legs_torque.data(), plain.Legs_torque.data(), 12 * B),
          "go1 tick %d set_bodies(nullptr)", tick);
  }
  CHECK(differ > 0, "go1: the rows changed no grf_opt");
  std::vector<double> rec((size_t)B * QLOCO_GO1_SERVO_STATE);
  fleet.get_state(rec.data());
  CHECK(all_finite(rec.data(), rec.size()), "go1: a refused row left a non-finite value in the member state");
  for (auto *p : one) delete p;
}

int main() {
  try {
    qloco_force_params base;
    qloco_force_params_default(&base);
    std::vector<qloco_force_body> rows(B);
    for (int b = 0; b < B; ++b) rows[b] = body(base, b % 4);
    test_dynamiccclass(rows);
    test_block(rows);
    test_go1(rows);
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

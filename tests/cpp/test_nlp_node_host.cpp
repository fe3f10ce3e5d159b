// test_nlp_node_host -- drives qloco::NLPRTControlBatch (include/qloco.hpp) for
// one robot as gait_nlp_kmp.cpp:101-158 drives NLPRTControlClass: per loop
// iteration a /rt2nrt/state row of 25 values from stdin, the counter and the
// latch advanced as the loop advances them, WalkingReactStepping while
// mpc_stop < 1.  Prints every row as hex floats ("T v0 .. v99") for
// tests/test_nlp_node_gpu.py, which compares them bit for bit with the Python
// path; checks here that the fleet form over device pointers gives the same
// rows for three robots, that a call out of the loop's order lands in the
// branch its counter asks for, and that get / set round-trips.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "qloco.hpp"

int main(int argc, char **argv) {
  const int ticks = argc > 1 ? atoi(argv[1]) : 45;
  const double stepheight = argc > 2 ? atof(argv[2]) : 0.0;
  try {
    qloco::NLPRTControlBatch one(1, stepheight), fleet(3, stepheight);
    qloco::DeviceArena ar;
    double *d_msg = (double *)ar.alloc(sizeof(double) * 3 * QLOCO_NRT_MSG_LEN);
    double *d_row = (double *)ar.alloc(sizeof(double) * 3 * QLOCO_GAIT_MSG_LEN);
    int32_t *d_sched = (int32_t *)ar.alloc(sizeof(int32_t) * 3 * QLOCO_NLP_NODE_SCHED_LEN);
    int count = 0;
    bool mpc_start = false;
    for (int t = 0; t < ticks; ++t) {
      double msg[3 * QLOCO_NRT_MSG_LEN];
      for (int k = 0; k < QLOCO_NRT_MSG_LEN; ++k)
        if (scanf("%lf", &msg[k]) != 1) return 2;
      for (int k = 0; k < QLOCO_NRT_MSG_LEN; ++k) msg[QLOCO_NRT_MSG_LEN + k] = msg[2 * QLOCO_NRT_MSG_LEN + k] = msg[k];
      if (msg[0] > 0) {
        mpc_start = true;
        count += 1;
      }
      const std::array<double, 100> row = one.WalkingReactStepping(count, mpc_start, msg + 1, msg + 22, msg + 19);
      if (row[98] != 0.0 || one.sched[5] != count || one.mpc_stop != row[97] || one.right_support != (int)row[99]) {
        printf("row / members disagree at tick %d\n", t);
        return 1;
      }
      const int want = !mpc_start ? QLOCO_NLP_NODE_NOT_STARTED : (count <= 40 ? QLOCO_NLP_NODE_SQUAT : QLOCO_NLP_NODE_WALKING);
      if (one.sched[0] != want || one.status != QLOCO_OK) {
        printf("branch %d (want %d), status %d at tick %d\n", one.sched[0], want, one.status, t);
        return 1;
      }
      ar.upload(d_msg, msg, sizeof(msg));
      ar.sync();
      fleet.tick(d_msg, d_row, d_sched, nullptr);
      fleet.sync();
      double rows[3 * QLOCO_GAIT_MSG_LEN];
      ar.download(rows, d_row, sizeof(rows));
      ar.sync();
      for (int b = 0; b < 3; ++b)
        for (int k = 0; k < QLOCO_GAIT_MSG_LEN; ++k) {
          const double g = rows[b * QLOCO_GAIT_MSG_LEN + k];
          if (!(g == row[k]) && !(std::isnan(g) && std::isnan(row[k]))) {
            printf("fleet robot %d slot %d differs at tick %d\n", b, k, t);
            return 1;
          }
        }
      printf("T");
      for (int k = 0; k < 100; ++k) printf(" %a", row[k]);
      printf("\n");
    }
    {  // out of the loop's order: the fifth squat tick as a first call
      qloco::NLPRTControlBatch jump(1, stepheight);
      const double z[18] = {0}, rf[3] = {0, -0.12675, 0}, lf[3] = {0, 0.12675, 0};
      const std::array<double, 100> row = jump.WalkingReactStepping(5, true, z, rf, lf);
      if (jump.sched[0] != QLOCO_NLP_NODE_SQUAT || jump.sched[1] != 5 || jump.sched[5] != 5 ||
          !(std::fabs(row[2] - jump.params.z_c) < 1e-12) || row[27] != 1.0) {
        printf("out-of-order call: branch %d, _walkdtime1 %d\n", jump.sched[0], jump.sched[1]);
        return 1;
      }
      jump.WalkingReactStepping(6, true, z, rf, lf);
      if (jump.sched[1] != 6 || jump.sched[5] != 6) {
        printf("the loop's step after an out-of-order call: _walkdtime1 %d\n", jump.sched[1]);
        return 1;
      }
    }
    std::vector<double> a(QLOCO_NLP_STATE), b(QLOCO_NLP_STATE), ta(QLOCO_NLP_TICK_STATE), tb(QLOCO_NLP_TICK_STATE);
    std::vector<double> na(QLOCO_NLP_NODE_STATE), nb(QLOCO_NLP_NODE_STATE);
    one.get_state(a.data(), ta.data(), na.data());
    one.set_state(a.data(), ta.data(), na.data());
    one.get_state(b.data(), tb.data(), nb.data());
    for (int k = 0; k < QLOCO_NLP_NODE_STATE; ++k)
      if (!(na[k] == nb[k]) && !(std::isnan(na[k]) && std::isnan(nb[k]))) {
        printf("node record element %d changed in a get / set round trip\n", k);
        return 1;
      }
    if (na[0] != count || a != b || ta != tb) {
      printf("records changed in a get / set round trip\n");
      return 1;
    }
    printf("ALL OK\n");
  } catch (const std::exception &e) {
    printf("exception: %s\n", e.what());
    return 1;
  }
  return 0;
}

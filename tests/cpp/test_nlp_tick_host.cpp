// test_nlp_tick_host -- drives qloco::NLPClassBatch (include/qloco.hpp) for one
// robot as NLPRTControlClass.cpp:445-459 drives NLPClass: ticks i = 1, 2, ..
// with the estimated state and the two foot-location feedbacks read from
// stdin (per tick: est[0..5], Rfoot x y, Lfoot x y), step_timing_opti_loop
// followed by Foot_trajectory_solve_mod2.  Prints per tick the 38-vector, the
// 18-vector and right_support as hex floats ("T v0 .. v37 | f0 .. f17 | rs")
// for tests/test_nlp_tick_gpu.py, which compares them bit for bit with the
// Python path; checks here that every slot is filled, that the foot call
// refuses another index and that get / set round-trips.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "qloco.hpp"

int main(int argc, char **argv) {
  const int ticks = argc > 1 ? atoi(argv[1]) : 10;
  const double stepheight = argc > 2 ? atof(argv[2]) : 0.0;
  try {
    qloco::NLPClassBatch nlp(1, 2 * 0.12675, 0.075, stepheight);
    for (int t = 0; t < ticks; ++t) {
      double est[18] = {0}, rf[3] = {0}, lf[3] = {0};
      for (int k = 0; k < 6; ++k)
        if (scanf("%lf", &est[k]) != 1) return 2;
      if (scanf("%lf %lf %lf %lf", &rf[0], &rf[1], &lf[0], &lf[1]) != 4) return 2;
      const std::array<double, 38> c = nlp.step_timing_opti_loop(t + 1, est, rf, lf, 0.0, false);
      const std::array<double, 18> f = nlp.Foot_trajectory_solve_mod2(t + 1, false);
      for (int k = 0; k < 38; ++k)
        if (std::isnan(c[k])) {
          printf("slot %d NaN at tick %d\n", k, t);
          return 1;
        }
      if (nlp.status()[0] != QLOCO_OK) {
        printf("status %d at tick %d\n", nlp.status()[0], t);
        return 1;
      }
      bool refused = false;
      try {
        nlp.Foot_trajectory_solve_mod2(t + 2, false);
      } catch (const std::exception &) {
        refused = true;
      }
      if (!refused) {
        printf("Foot_trajectory_solve_mod2 accepted another index at tick %d\n", t);
        return 1;
      }
      printf("T");
      for (int k = 0; k < 38; ++k) printf(" %a", c[k]);
      printf(" |");
      for (int k = 0; k < 18; ++k) printf(" %a", f[k]);
      printf(" | %d\n", nlp.right_support);
    }
    std::vector<double> a(QLOCO_NLP_STATE), b(QLOCO_NLP_STATE), ta(QLOCO_NLP_TICK_STATE), tb(QLOCO_NLP_TICK_STATE);
    nlp.get_state(a.data(), ta.data());
    nlp.set_state(a.data(), ta.data());
    nlp.get_state(b.data(), tb.data());
    for (int k = 0; k < QLOCO_NLP_STATE; ++k)
      if (!(a[k] == b[k])) {
        printf("record element %d changed in a get / set round trip\n", k);
        return 1;
      }
    for (int k = 0; k < QLOCO_NLP_TICK_STATE; ++k)
      if (!(ta[k] == tb[k])) {
        printf("second record element %d changed in a get / set round trip\n", k);
        return 1;
      }
    printf("ALL OK\n");
  } catch (const std::exception &e) {
    printf("exception: %s\n", e.what());
    return 1;
  }
  return 0;
}

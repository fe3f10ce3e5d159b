// test_nlp_host -- drives qloco::NLPStepTimingBatch (include/qloco.hpp) for
// one robot as NLPRTControlClass.cpp:445 drives NLPClass: ticks i = 1, 2, ..
// with the estimated state and the two foot-location feedbacks read from
// stdin (per tick: est[0..5], Rfoot x y, Lfoot x y).  Prints the 38-vector of
// every tick as hex floats ("T v0 .. v37") for tests/test_nlp_gpu.py, which
// compares them bit for bit with the Python path, and checks here that the
// slots the library does not compute are NaN and that get / set round-trips.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "qloco.hpp"

int main(int argc, char **argv) {
  const int ticks = argc > 1 ? atoi(argv[1]) : 10;
  try {
    qloco::NLPStepTimingBatch nlp(1, 2 * 0.12675, 0.075, 0.0);
    const int nan_slots[] = {2, 5, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 23, 26};
    for (int t = 0; t < ticks; ++t) {
      double est[18] = {0}, rf[3] = {0}, lf[3] = {0};
      for (int k = 0; k < 6; ++k)
        if (scanf("%lf", &est[k]) != 1) return 2;
      if (scanf("%lf %lf %lf %lf", &rf[0], &rf[1], &lf[0], &lf[1]) != 4) return 2;
      const std::array<double, 38> c = nlp.step_timing_opti_loop(t + 1, est, rf, lf, 0.0, false);
      for (int s : nan_slots)
        if (!std::isnan(c[s])) {
          printf("slot %d not NaN at tick %d\n", s, t);
          return 1;
        }
      if (nlp.status()[0] != QLOCO_OK) {
        printf("status %d at tick %d\n", nlp.status()[0], t);
        return 1;
      }
      printf("T");
      for (int k = 0; k < 38; ++k) printf(" %a", c[k]);
      printf("\n");
    }
    std::vector<double> a(QLOCO_NLP_STATE), b(QLOCO_NLP_STATE);
    nlp.get_state(a.data());
    nlp.set_state(a.data());
    nlp.get_state(b.data());
    for (int k = 0; k < QLOCO_NLP_STATE; ++k)
      if (!(a[k] == b[k])) {
        printf("record element %d changed in a get / set round trip\n", k);
        return 1;
      }
    printf("ALL OK\n");
  } catch (const std::exception &e) {
    printf("exception: %s\n", e.what());
    return 1;
  }
  return 0;
}

// test_go1_servo_host -- drives qloco::Go1ServoBatch (include/qloco.hpp) as
// servo.cpp's main loop drives its members: B robots, `ticks` iterations with
// the joint state, the IMU quaternion and the /MPC/Gait row read from stdin.
//   argv: batch ticks stand_duration t_walk_start t_period
//   stdin: B gait modes, B y_offsets, then per tick and robot q_mea[12],
//          quat[4], gait[100] (hex floats)
// Prints per tick and robot "T q_cmd[12] | state_to_MPC[25] | Legs_torque[12] |
// grf_opt[12] | FR..RL_angle_des[12] | joint2simulation[100]" as hex floats for
// tests/test_go1_servo_gpu.py, which compares them bit for bit with the Python
// path; checks here that n_count advances, that state_feedback(0) of one tick
// is the next tick's published row and that get / set round-trips.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "qloco.hpp"

int main(int argc, char **argv) {
  if (argc < 6) return 2;
  const int B = atoi(argv[1]), ticks = atoi(argv[2]);
  try {
    qloco_go1_servo_params prm;
    qloco_go1_servo_params_default(&prm);
    prm.stand_duration = atof(argv[3]);
    prm.t_walk_start = atof(argv[4]);
    prm.t_period = atof(argv[5]);
    qloco::Go1ServoBatch servo(B, &prm);
    std::vector<int32_t> mode(B);
    std::vector<double> yoff(B), q(B * 12), quat(B * 4), gait(B * 100), prev_fb(B, 0.0);
    for (int b = 0; b < B; ++b)
      if (scanf("%d", &mode[b]) != 1) return 2;
    for (int b = 0; b < B; ++b)
      if (scanf("%lf", &yoff[b]) != 1) return 2;
    for (int t = 0; t < ticks; ++t) {
      for (int b = 0; b < B; ++b) {
        for (int k = 0; k < 12; ++k)
          if (scanf("%lf", &q[12 * b + k]) != 1) return 2;
        for (int k = 0; k < 4; ++k)
          if (scanf("%lf", &quat[4 * b + k]) != 1) return 2;
        for (int k = 0; k < 100; ++k)
          if (scanf("%lf", &gait[100 * b + k]) != 1) return 2;
      }
      servo.tick(q.data(), quat.data(), gait.data(), mode.data(), yoff.data());
      if (servo.n_count != t + 1) {
        printf("n_count %d after tick %d\n", servo.n_count, t);
        return 1;
      }
      for (int b = 0; b < B; ++b) {
        if (servo.state_to_MPC[25 * b] != prev_fb[b]) {
          printf("robot %d tick %d: published t_int %g, previous state_feedback(0) %g\n", b, t,
                 servo.state_to_MPC[25 * b], prev_fb[b]);
          return 1;
        }
        prev_fb[b] = servo.state_feedback[25 * b];
        printf("T");
        for (int k = 0; k < 12; ++k) printf(" %a", servo.q_cmd[12 * b + k]);
        printf(" |");
        for (int k = 0; k < 25; ++k) printf(" %a", servo.state_to_MPC[25 * b + k]);
        printf(" |");
        for (int k = 0; k < 12; ++k) printf(" %a", servo.Legs_torque[12 * b + k]);
        printf(" |");
        for (int k = 0; k < 12; ++k) printf(" %a", servo.grf_opt[12 * b + k]);
        printf(" |");
        for (int k = 0; k < 3; ++k) printf(" %a", servo.FR_angle_des[3 * b + k]);
        for (int k = 0; k < 3; ++k) printf(" %a", servo.FL_angle_des[3 * b + k]);
        for (int k = 0; k < 3; ++k) printf(" %a", servo.RR_angle_des[3 * b + k]);
        for (int k = 0; k < 3; ++k) printf(" %a", servo.RL_angle_des[3 * b + k]);
        printf(" |");
        for (int k = 0; k < 100; ++k) printf(" %a", servo.joint2simulation[100 * b + k]);
        printf("\n");
      }
    }
    std::vector<double> a(B * QLOCO_GO1_SERVO_STATE), c(B * QLOCO_GO1_SERVO_STATE);
    servo.get_state(a.data());
    servo.set_state(a.data());
    servo.get_state(c.data());
    for (size_t k = 0; k < a.size(); ++k)
      if (!(a[k] == c[k])) {
        printf("record element %zu changed in a get / set round trip\n", k);
        return 1;
      }
    printf("ALL OK\n");
  } catch (const std::exception &e) {
    printf("exception: %s\n", e.what());
    return 1;
  }
  return 0;
}

// qloco_kin.hip -- batched Go1 leg kinematics: forward
// kinematics + Jacobian and damped-Newton inverse kinematics, fp64 like the
// reference, one leg per lane.
//
// Replaces Kinematicclass (go1_rt_control/src/kinematics/Kinematics.cpp); the
// device functions (and what they restate, line by line) are in
// qloco_kin_core.hpp, shared with the servo tick (qloco_go1_servo.hip).
//
// Memory: AoS fp64 rows (q / pos n*3, J n*9 col-major, leg n int32) are read
// and written by consecutive lanes, so a wave touches one contiguous span per
// array.  The FK kernel is HBM-bound (≈ 68 B in + 96 B out per leg with J);
// IK adds ≤ 15 FK evaluations + 3x3 solves per leg on the same traffic.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "qloco.h"
#include "qloco_common.hpp"
#include "qloco_kin_core.hpp"

namespace qloco {
namespace {

using namespace kin;  // leg_const, fk_local, body_rot, fk, cof3, ik_newton

__global__ __launch_bounds__(256) void leg_fk_kernel(int n, const double *__restrict__ q,
                                                     const int32_t *__restrict__ leg,
                                                     const double *__restrict__ body_p,
                                                     const double *__restrict__ body_r,
                                                     double *__restrict__ pos,
                                                     double *__restrict__ jac) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const LegConst k = leg_const(leg[i]);
  const bool global = body_p != nullptr;
  double R[9], P[3] = {0.0, 0.0, 0.0};
  if (global) {
    const double e[3] = {body_r[3 * i], body_r[3 * i + 1], body_r[3 * i + 2]};
    body_rot(e, R);
#pragma unroll
    for (int r = 0; r < 3; ++r) P[r] = body_p[3 * i + r];
  }
  const double qi[3] = {q[3 * i], q[3 * i + 1], q[3 * i + 2]};
  double p[3], J[9];
  fk(k, global, R, P, qi, p, J);
#pragma unroll
  for (int r = 0; r < 3; ++r) pos[3 * i + r] = p[r];
  if (jac) {
#pragma unroll
    for (int c = 0; c < 9; ++c) jac[9 * i + c] = J[c];
  }
}

__global__ __launch_bounds__(256) void leg_ik_kernel(
    int n, const double *__restrict__ pos_des, const double *__restrict__ q_ini,
    const int32_t *__restrict__ leg, const double *__restrict__ body_p,
    const double *__restrict__ body_r, double *__restrict__ q_out, double *__restrict__ pos,
    double *__restrict__ jac, int32_t *__restrict__ updates) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const LegConst k = leg_const(leg[i]);
  const bool global = body_p != nullptr;
  double R[9], P[3] = {0.0, 0.0, 0.0};
  if (global) {
    const double e[3] = {body_r[3 * i], body_r[3 * i + 1], body_r[3 * i + 2]};
    body_rot(e, R);
#pragma unroll
    for (int r = 0; r < 3; ++r) P[r] = body_p[3 * i + r];
  }
  const double pd[3] = {pos_des[3 * i], pos_des[3 * i + 1], pos_des[3 * i + 2]};
  double qd[3] = {q_ini[3 * i], q_ini[3 * i + 1], q_ini[3 * i + 2]};
  double p[3], J[9];
  fk(k, global, R, P, qd, p, J);
  const int nup = ik_newton(k, global, R, P, pd, qd, p, J);
#pragma unroll
  for (int r = 0; r < 3; ++r) q_out[3 * i + r] = qd[r];
  if (pos) {
#pragma unroll
    for (int r = 0; r < 3; ++r) pos[3 * i + r] = p[r];
  }
  if (jac) {
#pragma unroll
    for (int c = 0; c < 9; ++c) jac[9 * i + c] = J[c];
  }
  if (updates) updates[i] = nup;
}

}  // namespace
}  // namespace qloco

using namespace qloco;

extern "C" int qloco_leg_fk(int64_t n, const double *q, const int32_t *leg, const double *body_p,
                            const double *body_r, double *pos, double *jac, void *stream) {
  if (n < 0 || n > INT32_MAX || (n > 0 && (!q || !leg || !pos)) || ((body_p == nullptr) != (body_r == nullptr)))
    return QLOCO_ERR_ARG;
  if (n == 0) return QLOCO_OK;
  hipLaunchKernelGGL(leg_fk_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, (int)n, q, leg, body_p, body_r, pos, jac);
  QLOCO_HIP_CHECK(hipGetLastError(), "leg_fk_kernel launch");
  return QLOCO_OK;
}

extern "C" int qloco_leg_ik(int64_t n, const double *pos_des, const double *q_ini,
                            const int32_t *leg, const double *body_p, const double *body_r,
                            double *q_out, double *pos, double *jac, int32_t *updates,
                            void *stream) {
  if (n < 0 || n > INT32_MAX || (n > 0 && (!pos_des || !q_ini || !leg || !q_out)) ||
      ((body_p == nullptr) != (body_r == nullptr)))
    return QLOCO_ERR_ARG;
  if (n == 0) return QLOCO_OK;
  hipLaunchKernelGGL(leg_ik_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, (int)n, pos_des, q_ini, leg, body_p, body_r, q_out, pos,
                     jac, updates);
  QLOCO_HIP_CHECK(hipGetLastError(), "leg_ik_kernel launch");
  return QLOCO_OK;
}

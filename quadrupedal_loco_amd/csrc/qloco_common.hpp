// qloco_common.hpp -- shared device helpers for the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "qloco.h"

#define QLOCO_WAVE 64

// grouped force-QP dispatch (qloco_force.hip): 5 swing-leg patterns x 16
// iteration bins; the ordering workspace is 2 B + 2 kForceClasses int32
#define QLOCO_FORCE_CLASSES 80

namespace qloco {

// thread-local last HIP error (qloco_last_error)
void set_last_error(const char *where, hipError_t e);
// the same with a library message instead of a HIP error (RCCL, dlopen)
void set_last_error_msg(const char *where, const char *what);

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Make a value provably wave-uniform (SGPR) so branches on it stay scalar.
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float uni(float v) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

// OSQP limit_scaling (scaling.c): < MIN_SCALING -> 1, > MAX_SCALING -> MAX
__device__ __forceinline__ float limit_scaling(float d) {
  d = d < 1e-4f ? 1.0f : d;
  return d > 1e4f ? 1e4f : d;
}

// The qloco_force_body row rule (include/qloco.h section 3), stated once for
// qloco_force_body_check and the kernels of qloco_force.hip, qloco_servo.hip
// and qloco_go1_servo.hip.  r: the row's 16 doubles.
__host__ __device__ __forceinline__ bool force_body_ok(const double *r) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 16; ++k) ok = ok && isfinite(r[k]);
  ok = ok && r[0] > 0.0;  // mass
#pragma unroll
  for (int k = 1; k < 6; ++k) ok = ok && r[k] >= 0.0;  // alpha, beta, gamma, fz_max, mu
  return ok && r[15] == 0.0;  // reserved
}
static_assert(sizeof(qloco_force_body) == 128 && offsetof(qloco_force_body, momentum) == 48,
              "force_body_ok reads the row as 16 doubles");

// Momentum_sum, servo.cpp:375-377 (row-major): the constant of the two servo
// files and what qloco_force_body_from_params writes
#define QLOCO_MOMENTUM_SUM                                                                  \
  {2 * 0.0168352186, 2 * 0.0004636141, 2 * 0.0002367952, 2 * 0.0004636141, 2 * 0.0656071082, \
   2 * 3.6671e-05,   2 * 0.0002367952, 2 * 3.6671e-05,   2 * 0.0742720659}

// After the output copies of the force block and the servo tick: the caller's
// tau and grf_opt rows of every robot whose row is refused become NaN
// (qloco_force.hip).  rows != NULL.
int force_body_mark_refused(int64_t batch, const qloco_force_body *rows, double *tau,
                            double *grf_opt, hipStream_t stream);

}  // namespace qloco

#define QLOCO_HIP_CHECK(call, where)                   \
  do {                                                 \
    hipError_t _e = (call);                            \
    if (_e != hipSuccess) {                            \
      qloco::set_last_error(where, _e);                \
      return QLOCO_ERR_DEVICE;                         \
    }                                                  \
  } while (0)

// qloco_srbd_spec.hpp -- the SRBD horizon limits and the weights every SRBD
// entry point derives from a qloco_srbd_spec.  Plain C++: included by the HIP
// translation units and by the host table builder (qloco_srbd_tables.cpp).
#pragma once

#include "qloco.h"

namespace qloco {

constexpr int kMaxN = 20;  // max horizon compiled in (BASELINE configs: N <= 20)
// the literal QP through the wrench space (qloco_srbd_lit.hip): N <= kLitN on
// one wave, kLitN < N <= kLitN2 on two (each wave holds ceil(N / 2) steps)
constexpr int kLitN = 10;
constexpr int kLitN2 = 20;

// 2 * q_weights (Q diagonal, ConvexMpc.cpp:18-24) and 2 * r_weights (R
// diagonal, :38-45); r2 may be null
inline void srbd_doubled_weights(const qloco_srbd_spec *spec, float *q2, float *r2) {
  for (int k = 0; k < 13; ++k) q2[k] = 2.0f * spec->q_weights[k];
  if (r2)
    for (int k = 0; k < 12; ++k) r2[k] = 2.0f * spec->r_weights[k];
}

}  // namespace qloco

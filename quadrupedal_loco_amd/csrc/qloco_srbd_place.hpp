// qloco_srbd_place.hpp -- placement of the one-wave literal kernel's
// instances on SIMDs by the previous call's iteration counts.
//
// A launch of B one-wave workgroups with S < B <= 4 S (S = SIMDs of the
// device) is resident from its first cycle, workgroup p on SIMD p mod S.  The
// launch ends with its most loaded SIMD, and a SIMD's longest instance
// finishes alone, so the longest instances are spread one per SIMD and each
// is given the shortest instances left as companions.
//
// State (int32 words, the caller's, valid when zeroed):
//   [0]                     ready: == batch once order[] holds a permutation
//   [1, kPlaceHeader)       zero
//   hint[batch]             iteration count of each instance's last solve
//   order[batch]            workgroup position -> instance
#pragma once
#include <stdint.h>

#include "qloco_common.hpp"

namespace qloco {

constexpr int kPlaceHeader = 4;
constexpr int kPlaceClasses = 256;

// Iteration counts differ in steps of check_termination: one class per check,
// the longest in class 255.  Any word is a class (negative -> 0).
__host__ __device__ inline int place_class(int hint, int check_termination) {
  const int c = hint / (check_termination > 1 ? check_termination : 1);
  return c < 0 ? 0 : (c > kPlaceClasses - 1 ? kPlaceClasses - 1 : c);
}

// Rank (0 = longest) of the instance at workgroup position p, S < B <= 4 S.
// Position p = s + S q runs on SIMD s as its q-th workgroup.  q = 0: rank s,
// the heads.  The T = B - S others are handed out from the short end, SIMD
// s's companions next to each other: m = ceil(T / S) on the first
// r = T - (m - 1) S SIMDs, m - 1 on the rest.  A bijection of [0, B).
__host__ __device__ inline int64_t place_rank(int64_t p, int64_t B, int64_t S) {
  const int64_t s = p % S, q = p / S;
  if (q == 0) return s;
  const int64_t T = B - S, m = (T + S - 1) / S, r = T - (m - 1) * S;
  return B - 1 - (s * (m - 1) + (s < r ? s : r) + (q - 1));
}

// Its inverse: the position of rank k.
__host__ __device__ inline int64_t place_position(int64_t k, int64_t B, int64_t S) {
  if (k < S) return k;
  const int64_t T = B - S, m = (T + S - 1) / S, r = T - (m - 1) * S;
  const int64_t j = B - 1 - k;  // index from the short end, [0, T)
  int64_t s, c;
  if (j < r * m) {
    s = j / m;
    c = j - s * m;
  } else {
    const int64_t jj = j - r * m;  // m >= 2 here: m = 1 has r = T
    s = r + jj / (m - 1);
    c = jj - (s - r) * (m - 1);
  }
  return s + S * (c + 1);
}

}  // namespace qloco

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
//   order[batch]            the instance of rank k at order[place_position(k)]
//
// Which rank a workgroup takes is the solve kernel's choice (place_assign,
// DESIGN.md §3r): it never reads hint[], which its own launch overwrites.
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

// Rank that the workgroup at position p = s + S q solves:
// the solve kernel reads order[place_position(place_assign(p))].  order[] and
// place_rank keep their meaning; this map alone decides which ranks share a
// SIMD.  Rank-only integer arithmetic, a bijection of [0, B) for S < B <= 4 S.
//
// q = 0: rank s, as before: the S longest one per SIMD, each SIMD's first
// workgroup.  The companions, ranks S .. B - 1, with m = ceil((B - S) / S)
// rows of them, the last one on the first r SIMDs only:
//   m = 1, or s < A1 = S / 64   place_rank: the shortest left, next to each
//                               other (a head far above the rest ends its
//                               SIMD alone whatever joins it)
//   A1 <= s < A2 = 3 S / 16     q = 1: one of the longest companions; the
//                               other rows: the shortest left, next to each
//                               other
//   s >= A2                     one companion of each stratum: q = 1 of the
//                               longest, row m of the shortest left, the rows
//                               between of the strata between
// In every row a longer head takes a shorter companion.  place_rank gave the
// short heads, most of the SIMDs, companions of one class, their own.
__host__ __device__ inline int64_t place_assign(int64_t p, int64_t B, int64_t S) {
  const int64_t s = p % S, q = p / S;
  if (q == 0) return s;
  const int64_t T = B - S, m = (T + S - 1) / S, r = T - (m - 1) * S;
  const int64_t A1 = m < 2 ? S : S / 64, A2 = A1 > 3 * S / 16 ? A1 : 3 * S / 16;
  const int64_t n2 = A2 - A1, n3 = S - A2;
  // companions of the SIMDs before s: m on the first r, m - 1 on the rest
  const int64_t before = s * (m - 1) + (s < r ? s : r);
  if (s < A1) return B - 1 - (before + (q - 1));
  if (s < A2) {
    // ranks [S, S + n3) are zone three's q = 1 row, [S + n3, S + n3 + n2) this zone's
    if (q == 1) return S + n3 + (A2 - 1 - s);
    return B - 1 - (before - (s - A1) + (q - 2));
  }
  const int64_t i = s - A2;
  if (q == 1) return S + (n3 - 1 - i);
  // from the short end: what zones one and two took, row m's stratum (on the
  // SIMDs of this zone that have a row m), then rows m - 1 .. 2
  const int64_t taken = A2 * (m - 1) + (A2 < r ? A2 : r) - n2;
  if (q == m) return B - 1 - (taken + i);
  const int64_t last = r - A2 < 0 ? 0 : (r - A2 > n3 ? n3 : r - A2);
  return B - 1 - (taken + last + (m - 1 - q) * n3 + i);
}

}  // namespace qloco

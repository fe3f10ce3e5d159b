// qloco_srbd_model.hpp -- the single-rigid-body model of ConvexMpc.cpp:111-160
// / compute_grf (A1RobotControl.cpp:502-549), stated once for the SRBD kernels
// (qloco_srbd.hip and its wide path qloco_srbd_big.inc, qloco_srbd_lit.hip,
// qloco_srbd_build.hip), and the instance prologue the stance-only one- / two-
// wave kernel and the wide kernel share.  Leaf functions only: no LDS layout
// and no kernel structure in a signature; the prologue functions take the
// LDS struct as a template parameter and leave every barrier to the caller.
// DESIGN.md §3p has the per-kernel record; §3s the per-instance body (srbd_body).
#pragma once

#include <math.h>

#include "qloco_srbd_core.hpp"

namespace qloco {

// The body of one instance: the five quantities of qloco_srbd_model
struct SrbdBody {
  float mass;
  float inertia[9];
  float mu, fz_min, fz_max;
};

// Instance b's body: its row of a.model (qloco_srbd_model, 16 floats) when
// the call carries rows, the kernel-argument fields otherwise.  b is
// wave-uniform in every SRBD kernel (a blockIdx expression, or a uniform load
// from the class list / the placement order), so the row arrives by scalar
// loads: the index through readfirstlane, the row read through the constant
// address space (the rows are never written during a call), and the values
// stay in SGPRs like the kernel arguments they replace.  The 13 floats are
// adjacent dword loads of a 64-byte-aligned row, merged by the compiler; a
// caller that uses some of them gets those loads alone.
template <class Args>
__device__ __forceinline__ SrbdBody srbd_body(const Args &a, int64_t b) {
  SrbdBody m;
  if (a.model) {
    typedef const __attribute__((address_space(4))) float *row_ptr;
    const int64_t bu = ((int64_t)__builtin_amdgcn_readfirstlane((int)(b >> 32)) << 32) |
                       (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
    const row_ptr r = (row_ptr)(uintptr_t)__builtin_assume_aligned(a.model + 16 * bu, 64);
    m.mass = r[0];
#pragma unroll
    for (int k = 0; k < 9; ++k) m.inertia[k] = r[1 + k];
    m.mu = r[10];
    m.fz_min = r[11];
    m.fz_max = r[12];
  } else {
    m.mass = a.mass;
#pragma unroll
    for (int k = 0; k < 9; ++k) m.inertia[k] = a.inertia[k];
    m.mu = a.mu;
    m.fz_min = a.fz_min;
    m.fz_max = a.fz_max;
  }
  return m;
}

// The same quantities for a kernel with one instantiation per kind of call
// (the literal kernels): ROWS = true reads the row srbd_body loaded, ROWS =
// false the kernel-argument field itself, at the place of use, so that
// instantiation compiles as a kernel that knows no rows does.
template <bool ROWS>
struct SrbdBodyAt {
  const SrbdArgs &a;
  SrbdBody row;  // ROWS only
  __device__ __forceinline__ float mass() const { return ROWS ? row.mass : a.mass; }
  __device__ __forceinline__ const float *inertia() const { return ROWS ? row.inertia : a.inertia; }
  __device__ __forceinline__ float mu() const { return ROWS ? row.mu : a.mu; }
  __device__ __forceinline__ float fz_min() const { return ROWS ? row.fz_min : a.fz_min; }
  __device__ __forceinline__ float fz_max() const { return ROWS ? row.fz_max : a.fz_max; }
};

// A row the solve refuses (qloco_srbd_solve_model): one of its 13 values is
// not finite, or mass <= 0.  Asked of rows only: the kernel-argument body is
// validated on the host, as before.
__device__ __forceinline__ bool srbd_body_bad(const SrbdBody &m) {
  bool ok = m.mass > 0.0f && isfinite(m.mass) && isfinite(m.mu) && isfinite(m.fz_min) &&
            isfinite(m.fz_max);
#pragma unroll
  for (int k = 0; k < 9; ++k) ok = ok && isfinite(m.inertia[k]);
  return !ok;
}

// World inverse inertia (Rz I Rz')^-1 with the yaw "rotation"
// R = [[c,s,0],[-s,c,0],[0,0,1]] that overwrites root_rot_mat
// (A1RobotControl.cpp:502-510); I row-major.  The caller evaluates cos / sin
// (DESIGN.md §3l pins their bits per kernel).
__device__ __forceinline__ void srbd_inertia_inv(float cy, float sy, const float *I,
                                                 float (&Ii)[3][3]) {
  const float Rm[3][3] = {{cy, sy, 0.f}, {-sy, cy, 0.f}, {0.f, 0.f, 1.f}};
  float RI[3][3], Iw[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      RI[r][c] = Rm[r][0] * I[c * 3 + 0] + Rm[r][1] * I[c * 3 + 1] + Rm[r][2] * I[c * 3 + 2];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      Iw[r][c] = RI[r][0] * Rm[c][0] + RI[r][1] * Rm[c][1] + RI[r][2] * Rm[c][2];
  const float c00 = Iw[1][1] * Iw[2][2] - Iw[1][2] * Iw[2][1];
  const float c01 = Iw[1][2] * Iw[2][0] - Iw[1][0] * Iw[2][2];
  const float c02 = Iw[1][0] * Iw[2][1] - Iw[1][1] * Iw[2][0];
  const float id = 1.0f / (Iw[0][0] * c00 + Iw[0][1] * c01 + Iw[0][2] * c02);
  Ii[0][0] = c00 * id;
  Ii[1][0] = c01 * id;
  Ii[2][0] = c02 * id;
  Ii[0][1] = (Iw[0][2] * Iw[2][1] - Iw[0][1] * Iw[2][2]) * id;
  Ii[1][1] = (Iw[0][0] * Iw[2][2] - Iw[0][2] * Iw[2][0]) * id;
  Ii[2][1] = (Iw[0][1] * Iw[2][0] - Iw[0][0] * Iw[2][1]) * id;
  Ii[0][2] = (Iw[0][1] * Iw[1][2] - Iw[0][2] * Iw[1][1]) * id;
  Ii[1][2] = (Iw[0][2] * Iw[1][0] - Iw[0][0] * Iw[1][2]) * id;
  Ii[2][2] = (Iw[0][0] * Iw[1][1] - Iw[0][1] * Iw[1][0]) * id;
}

// Foot position of (step, leg) in instance b: feet is (B, 12) or, per step,
// (B, N, 12)
__device__ __forceinline__ const float *srbd_foot(const float *feet, int64_t b, int N,
                                                  int feet_per_step, int step, int leg) {
  return feet + b * (feet_per_step ? 12 * N : 12) + (feet_per_step ? 12 * step : 0) + 3 * leg;
}

// One force component's column of B_d (ConvexMpc.cpp:135-147) and of
// E = dt A_c B_d: ba = dt I_w^-1 skew(r) e_comp (rows 6..8 of B_d), packed
// with E's rows 0..2 as lo = {ba, e0}, hi = {e1, e2, step, comp}.  Lanes
// without a variable get zeros and comp = -1.
__device__ __forceinline__ void srbd_bd_column(const float (&Ii)[3][3], const float *rf, int comp,
                                               float dt, float R00, float R01, float R10,
                                               float R11, int step, bool valid, float (&ba)[3],
                                               f4v &lo, f4v &hi) {
  const float rx = rf[0], ry = rf[1], rz = rf[2];
  const float tv0 = comp == 0 ? 0.f : (comp == 1 ? -rz : ry);  // skew(r) e_comp (Utils.cpp:35-41)
  const float tv1 = comp == 0 ? rz : (comp == 1 ? 0.f : -rx);
  const float tv2 = comp == 0 ? -ry : (comp == 1 ? rx : 0.f);
#pragma unroll
  for (int r = 0; r < 3; ++r) ba[r] = dt * (Ii[r][0] * tv0 + Ii[r][1] * tv1 + Ii[r][2] * tv2);
  lo = (f4v){ba[0], ba[1], ba[2], dt * (R00 * ba[0] + R01 * ba[1])};
  hi = (f4v){dt * (R10 * ba[0] + R11 * ba[1]), dt * ba[2], (float)step, (float)comp};
  if (!valid) {
    lo = (f4v)(0.0f);
    hi = (f4v){0.0f, 0.0f, 0.0f, -1.0f};
  }
}

// State row s of the free response A_d^{i+1} x0 in closed form (A_c is
// nilpotent).  NX = 12: the solve kernels' rows (the gravity state enters
// through rows 5 and 11 only); NX = 13: the dense build's, with the gravity
// state's own row
template <int NX>
__device__ __forceinline__ float srbd_free_state(const float *x0, int s, int i, float dt,
                                                 float R00, float R01, float R10, float R11) {
  const float k = (float)(i + 1);
  float xf;
  if (s < 3) {
    const float rw = s == 0 ? (R00 * x0[6] + R01 * x0[7]) : (s == 1 ? (R10 * x0[6] + R11 * x0[7]) : x0[8]);
    xf = x0[s] + k * dt * rw;
  } else if (s < 6) {
    xf = x0[s] + k * dt * x0[s + 6];
    if (s == 5) xf += 0.5f * k * (k - 1.0f) * dt * dt * x0[12];
  } else if (s < 9) {
    xf = x0[s];
  } else if (NX == 12 || s < 12) {
    xf = x0[s] + (s == 11 ? k * dt * x0[12] : 0.0f);
  } else {
    xf = x0[12];
  }
  return xf;
}

// ---- the instance prologue of srbd_solve_one<W> and srbd_admm_big_kernel.
// NT: threads of the workgroup; Lds: SrbdLds<W, NM> or BigLds.

// x0, the doubled weights and the contact flags -> LDS
template <int NT, class Lds>
__device__ __forceinline__ void srbd_load_inputs(const SrbdArgs &a, Lds &S, int64_t b, int t) {
  const int N = a.N;
  if (t < 13) S.x0[t] = a.x0[b * 13 + t];
  if (t == 0) {  // static indices: kernel-argument arrays never indexed per lane
#pragma unroll
    for (int k = 0; k < 13; ++k) S.q2[k] = a.q2[k];
#pragma unroll
    for (int k = 0; k < 12; ++k) S.r2[k] = a.r2[k];
  }
  const int nct = a.contacts_per_step ? 4 * N : 4;
  for (int k = t; k < 4 * N; k += NT)
    S.ct[k] = a.contacts[b * nct + (a.contacts_per_step ? k : (k & 3))] ? 1 : 0;
}

// Variable enumeration (integer, bit-exact) by wave 0: the stance
// (step, leg) pairs in order, or every pair for the literal full QP, into
// S.legtab; their count into S.nlegs; the pairs before each step into
// S.stepstart
template <class Lds>
__device__ __forceinline__ void srbd_enumerate_stance(const SrbdArgs &a, Lds &S, int t) {
  const int N = a.N;
  const int wave = t >> 6, lane = t & 63;
  if (wave == 0) {
    const bool s0 = (lane < 4 * N) && (a.literal || S.ct[lane]);
    const bool s1 = (64 + lane < 4 * N) && (a.literal || S.ct[64 + lane]);
    const uint64_t m0 = __ballot(s0), m1 = __ballot(s1);
    const uint64_t below = (1ull << lane) - 1ull;
    const int c0 = __popcll(m0);
    if (s0) S.legtab[__popcll(m0 & below)] = lane;
    if (s1) S.legtab[c0 + __popcll(m1 & below)] = 64 + lane;
    if (lane == 0) S.nlegs = c0 + __popcll(m1);
    if (lane <= N) {
      const int q = 4 * lane;
      const uint64_t l0 = q >= 64 ? ~0ull : ((1ull << q) - 1ull);
      const int q1 = q - 64;
      const uint64_t l1 = q1 <= 0 ? 0ull : ((1ull << q1) - 1ull);
      S.stepstart[lane] = __popcll(m0 & l0) + __popcll(m1 & l1);
    }
  }
}

// The result of an instance the kernel does not solve: the code as its status
// and NaN outputs.  QLOCO_BAD_SIZE: more stance legs than the kernel holds
// (the caller's max_stance_legs was too small); QLOCO_ERR_ARG: an invalid
// model row (srbd_body_bad)
template <int NT>
__device__ __forceinline__ void srbd_refuse(const SrbdArgs &a, int64_t b, int t, int code) {
  const int N = a.N;
  if (t < 12) a.u0[b * 12 + t] = NAN;
  if (a.u)
    for (int k = t; k < 12 * N; k += NT) a.u[b * 12 * N + k] = NAN;
  if (t == 0) {
    if (a.status) a.status[b] = code;
    if (a.iters) a.iters[b] = 0;
    if (a.hint) a.hint[b] = 0;  // placement state (the one-wave literal kernel)
    if (a.rho_updates) a.rho_updates[b] = 0;
    if (a.obj) a.obj[b] = NAN;
  }
}

// Persistent solver (warm_start == 2, A1RobotControl.cpp:556-578): the record
// of this instance's last call (layout: QLOCO_SRBD_PERSIST_LEN), or null.
// p_init: the record holds a solve; p_same: it takes OSQP's update path.  The
// literal full QP's structure never changes (the reference's Hessian pattern
// is contact-independent, ConvexMpc.cpp:211-215), so every call after the
// first takes the update path; the stance-only reduction re-initialises when
// its variable set changes.  Every thread of the block
// calls it: it holds a block-wide vote when a record is in use.
template <int NT, bool WS, class Lds>
__device__ __forceinline__ float *srbd_persist_record(const SrbdArgs &a, const Lds &S, int64_t b,
                                                      int t, bool &p_init, bool &p_same) {
  const int N = a.N;
  const int NP = 100 * N;
  float *prec = (WS && a.warm_start == 2) ? a.warm + b * (int64_t)(NP + 4) : nullptr;
  p_init = false;
  p_same = false;
  if (prec) {
    p_init = prec[NP + 1] > 0.5f;
    int mism = 0;
    if (!a.literal)
      for (int k = t; k < 4 * N; k += NT) mism |= (prec[96 * N + k] != 0.0f) != (S.ct[k] != 0);
    p_same = p_init && !__syncthreads_or(mism);
  }
  return prec;
}

}  // namespace qloco

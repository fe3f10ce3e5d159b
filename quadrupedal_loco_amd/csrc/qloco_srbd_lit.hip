// qloco_srbd_lit.hip -- the reference's LITERAL 12N-variable SRBD QP for
// N <= 20 (every (step, leg) pair an ADMM variable, swing legs held by their
// fz in [0, 0] rows: A1RobotControl.cpp:557-578, ConvexMpc.cpp:162-264),
// the OSQP linear solve through the per-step wrench space, one wavefront per
// instance for N <= 10 and two for 11 <= N <= 20 (dispatched by
// qloco_srbd_solve_ex, qloco_srbd.hip).
//
// Why the wrench space.  The forces enter the SRBD dynamics
// only through each step's wrench increment w_j = Bb u_j (Bb: the omega / v
// rows of B_d, 6 x 12), so the condensed Hessian is H = Vu' G Vu + R with
// Vu = I_N (x) Bb and G = K0 (x) Qb + K2 (x) Te (6N x 6N, the closed-form
// horizon sums of DESIGN.md §3).  OSQP's reduced KKT matrix factors as
//   K = P~ + sigma I + A~' rho A~ = D [c Vu' G Vu + W0] D,
//   W0 = c R + D^-1 (sigma I + A~' rho A~) D^-1   (3 x 3 per (step, leg)),
// and by the push-through identity
//   K^-1 b = D^-1 (a - W0^-1 Vu' T Vu a),  a = W0^-1 D^-1 b,
//   T = (I + cG U)^-1 cG = (cG) L S^-1 L^-1   (symmetric, 6N x 6N),
//   U = Vu W0^-1 Vu' = L L' (6 x 6 per step),  S = I + L' (cG) L  (SPD, >= I).
// The 12N-variable KKT inverse becomes a 6N x 6N inverse of the
// well-conditioned S (eigenvalues >= 1, so pivot-free Gauss-Jordan is
// stable) plus a 6N x 6N product, and each ADMM iteration a 6N x 6N matvec
// plus leg-local 3 x 3 blocks and per-step wrench sums.  Same arithmetic as
// OSQP up to rounding (tools/proto_lit.py: float64 iterates agree to 1e-10,
// a float32 solve to 4e-7 relative; iteration counts equal on every instance
// tried).
//
// Lane layout (template W = waves per instance).  Wave w holds the steps
// [w H, w H + N_w) (W = 1: H = N_0 = N; W = 2: H = ceil(N / 2), N_1 = N - H,
// at most 10 steps a wave), laid out exactly as the one-wave kernel lays out
// its N <= 10 steps: lane l holds two variables (slot h = 0, 1: local
// v = 60 h + l, l < 60; step w H + v / 12, leg (v % 12) / 3, component
// v % 3 -- leg triples never straddle), their <= 2 constraint rows each,
// and wrench row l (step w H + l / 6, component l % 6: 0..2 omega, 3..5 v).
// Everything leg- or step-local stays inside a wave; the couplings across
// steps (the K0 / K2 horizon sums, the rows of S and T, the matvec with T)
// run in a "column space" of W halves of 60 (half w' = wave w''s wrench rows),
// so a lane's row of S / T is 60 W registers and the Gauss-Jordan and the
// matvec are W of the one-wave kernel's 60-column DPP forms.
#include <math.h>
#include <stddef.h>

#include <type_traits>

#include "qloco_srbd_core.hpp"
#include "qloco_srbd_model.hpp"
#include "qloco_srbd_place.hpp"

namespace qloco {

constexpr int kLitWpe = 4;   // one wave:  waves per SIMD: 128 VGPRs, <= 10 KB of LDS (static_assert below)
constexpr int kLit2Wpe = 2;  // two waves: 256 VGPRs (a 120-register row of S / T per lane)

template <int W>
struct LitLds {
  // steps the per-step loops unroll over; the per-step tables (K0 / K2, Ruiz
  // column scales) are indexed by COLUMN-SPACE step 10 w' + kl
  // (wave w''s local step kl; two waves: the steps past a wave's N_w are
  // padding with zero K0 / K2 weights), so every table index in the unrolled
  // loops is a compile-time constant plus the wave's offset
  static constexpr int NS = W == 1 ? kLitN : kLitN2;
  static constexpr int NT = NS;
  // Member order: the ADMM iteration addresses LDS from a few
  // loop-invariant lane registers, and the two-address reads reach 255 dwords
  // (ds_read2_b32) or 255 x 256 B (ds_read2st64_b32) from them.  The small
  // constant tables come first (768 B for one wave, padded to 1024 B for two:
  // the Bb columns within a ds_read2_b32 of 4 (lane % 12)), and every per-lane
  // array of the loop, the union's w0i included, then starts a multiple of
  // 256 B after bc: one register 4 lane serves them all with immediate offsets.
  float Bb[6][12];          // wrench map (constant feet), rows omega 0..2, v 3..5 (rows read as f4v)
  float Te[6][6];           // dt^2 blockdiag(Rz' Qtheta Rz, Qp)
  float q2[16], r2[12], x0[16];
  float ctf[4 * NT];        // contact flags as floats
  float pad0[W == 1 ? 0 : 24];
  f4v bc[W][W][16];         // broadcast rows: 60-vectors read as one 16-B chunk per lane, [parity][half]
                            // (one wave: its LDS ops run in order, so one buffer serves every reuse;
                            // two waves: double-buffered by iteration / pivot parity, one barrier each)
  float av[W][2][64];       // per wave, per slot exchange (a, D x, t)
  float wv[W][64];          // per wave, wrench rows (s, w)
  float zh[W][2][64];       // per slot: row 0's scaled upper bound (x / y rows: inf); the lower
                            // bound is 0 (x / y) or zh fz_min / fz_max (z rows)
  float dr[W][2][64];       // per slot: the Ruiz column scale D (read where needed: not a
                            // register live across the ADMM loop)
  float qvl[W][2][64];      // per slot: the scaled gradient q~ (read where needed)
  f4v arz[W][2][64];        // per slot: scaled A entries (ra0, ra1, rz0, rz1)
  union alignas(16) {       // phase-local storage (LDS bounds the one-wave occupancy: <= 10 KB;
                            // 16-byte aligned: dcol is read as f4v, a misaligned ds_read_b128
                            // cost the one-wave kernel 46 us per launch)
    struct {                // gradient + Ruiz
      f2v beps[12][12];     // (beta, eps)[w][w']: the P entries' per-column coefficients
      float dcol[12 * NT];  // Ruiz column scales D (read as same-address broadcasts)
      float err[12 * NT];   // gradient scans
      float Wc[12 * NT];
    };
    struct {                // factorisation
      float w0i[W][3][2][64];   // per variable its row of W0^-1 (x, y, z), read by the U rows; between
                                // two factorisations the ADMM segments park D^-1 in [0] and the
                                // first rows' lower bound in [1]
      f2v gtab[NT][NT][3];      // G^-1 blocks: per (row step, column step) in
                                // column-space order, (W0, W1), (W2, V0), (V1, V2)
    };
  };
  f2v k0k2[NT][NT];         // horizon sums K0 / K2 (row step, column step; column-space steps)
  // block-uniform solver state, one copy per wave (both waves take identical
  // decisions): read into SGPRs where a phase needs it, so no register carries
  // it across the ADMM iterations
  struct {
    float rho, cs, cinv, qn0, qn1, alpha, oma, sigma, dtm;
    float zlo;        // fz_min / fz_max: the z rows' lower bound is zlo times the upper one
    float sxy[2][2];  // S of the omega x / y block: G^-1 = sum_a S[.][a] A_a^-1 S[.][a] (see the G^-1 tables)
    int iter, status, rho_updates, ctm, interval;
  } sc[W];
  float piv[W == 1 ? 0 : 2];       // two waves: the Gauss-Jordan pivot, [parity]
  float red[W == 1 ? 0 : 2][16];   // two waves: per-wave partials of the block reductions
};
static_assert(sizeof(LitLds<1>) <= 10240, "literal kernel: four workgroups per SIMD need <= 160 KB / 16 of LDS");
static_assert(sizeof(LitLds<2>) <= 40960, "two-wave literal kernel: four workgroups per CU need <= 40 KB");
static_assert(offsetof(LitLds<1>, dcol) % 16 == 0 && offsetof(LitLds<2>, dcol) % 16 == 0,
              "dcol is read as f4v (ds_read_b128 needs 16-byte alignment)");
static_assert(offsetof(LitLds<1>, Bb) % 16 == 0 && offsetof(LitLds<1>, bc) % 16 == 0 && offsetof(LitLds<1>, arz) % 16 == 0 &&
                  offsetof(LitLds<2>, Bb) % 16 == 0 && offsetof(LitLds<2>, bc) % 16 == 0 && offsetof(LitLds<2>, arz) % 16 == 0,
              "Bb rows, bc and arz are read as f4v");
static_assert((offsetof(LitLds<1>, w0i) - offsetof(LitLds<1>, bc)) % 256 == 0 &&
                  (offsetof(LitLds<2>, w0i) - offsetof(LitLds<2>, bc)) % 256 == 0 && offsetof(LitLds<1>, Bb) == 0,
              "the ADMM loop's two-address reads reach its per-lane arrays from one lane register");

// Wave-level helpers for the one-wave literal kernel
__device__ __forceinline__ void lsync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// the instance's workgroup: a wave barrier for one wave, s_barrier for two
template <int W>
__device__ __forceinline__ void bsync() {
  if constexpr (W == 1)
    lsync();
  else
    __syncthreads();
}

// Block-wide combination of W wave-uniform partials (fixed order: every wave
// computes the same value bit for bit, so the loop control stays uniform)
template <int W, int K>
__device__ __forceinline__ void bcombine_max(LitLds<W> &S, float (&v)[K], int wv) {
  if constexpr (W == 2) {
    static_assert(K <= 16, "red holds 16 partials per wave");
    if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0) {
#pragma unroll
      for (int k = 0; k < K; ++k) S.red[wv][k] = v[k];
    }
    bsync<W>();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = fmaxf(S.red[0][k], S.red[1][k]);
    bsync<W>();
  }
}
template <int W>
__device__ __forceinline__ float bsum(LitLds<W> &S, float v, int wv) {
  if constexpr (W == 2) {
    if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0) S.red[wv][0] = v;
    bsync<W>();
    v = S.red[0][0] + S.red[1][0];
    bsync<W>();
  }
  return v;
}
template <int W>
__device__ __forceinline__ float bmax1(LitLds<W> &S, float v, int wv) {
  float t[1] = {v};
  bcombine_max<W, 1>(S, t, wv);
  return t[0];
}

// The three entries of this lane's leg triple (components 0, 1, 2) of a
// per-lane value: lanes 3m, 3m+1, 3m+2 hold one leg.
struct Triple {
  float v0, v1, v2;
};
__device__ __forceinline__ Triple triple(float v, int comp) {
  const float n1 = lane_next(v), n2 = lane_next(n1);
  const float p1 = lane_prev(v), p2 = lane_prev(p1);
  Triple t;
  t.v0 = comp == 0 ? v : (comp == 1 ? p1 : p2);
  t.v1 = comp == 0 ? n1 : (comp == 1 ? v : p1);
  t.v2 = comp == 0 ? n2 : (comp == 1 ? n1 : v);
  return t;
}

// A leg-triple dot product sum_j a_j v(leg, j) as lane shifts d = j - comp:
// v(l + d) with coefficient c_d (zero where l + d leaves the leg), five fused
// multiply-adds with DPP operands instead of the triple's 4 moves + 6 selects
// + 3 multiply-adds.
struct Shift5 {
  float cm2, cm1, c0, cp1, cp2;
};
__device__ __forceinline__ Shift5 shift5(float a0, float a1, float a2, int comp) {
  Shift5 c;
  c.c0 = comp == 0 ? a0 : (comp == 1 ? a1 : a2);
  c.cm1 = comp == 1 ? a0 : (comp == 2 ? a1 : 0.0f);
  c.cm2 = comp == 2 ? a0 : 0.0f;
  c.cp1 = comp == 0 ? a1 : (comp == 1 ? a2 : 0.0f);
  c.cp2 = comp == 0 ? a2 : 0.0f;
  return c;
}
__device__ __forceinline__ float tdot(float v, const Shift5 &c) {
  float a, t, u;
  asm("s_nop 1\n\t"
      "v_mov_b32_dpp %1, %3 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_mov_b32_dpp %2, %3 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_mul_f32 %0, %3, %4\n\t"
      "v_fmac_f32_dpp %0, %3, %5 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_fmac_f32_dpp %0, %3, %7 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_fmac_f32_dpp %0, %1, %6 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_fmac_f32_dpp %0, %2, %8 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:0"
      : "=&v"(a), "=&v"(t), "=&v"(u)
      : "v"(v), "v"(c.c0), "v"(c.cm1), "v"(c.cm2), "v"(c.cp1), "v"(c.cp2));
  return a;
}

// Two independent tdots, term by term side by side (each one's operations in
// tdot's order, so the same bits): a DPP operand is read two or more
// instructions after it is written, and one pad covers both inputs.
__device__ __forceinline__ void tdot2(float v0, const Shift5 &c, float v1, const Shift5 &d, float &a0, float &a1) {
  float t0, t1, u0, u1;
  asm("s_nop 1\n\t"
      "v_mov_b32_dpp %2, %6 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_mov_b32_dpp %3, %7 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_mov_b32_dpp %4, %6 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_mov_b32_dpp %5, %7 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_mul_f32 %0, %6, %8\n\t"
      "v_mul_f32 %1, %7, %13\n\t"
      "v_fmac_f32_dpp %0, %6, %9 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_fmac_f32_dpp %1, %7, %14 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_fmac_f32_dpp %0, %6, %11 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_fmac_f32_dpp %1, %7, %16 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_fmac_f32_dpp %0, %2, %10 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_fmac_f32_dpp %1, %3, %15 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_fmac_f32_dpp %0, %4, %12 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
      "v_fmac_f32_dpp %1, %5, %17 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:0"
      : "=&v"(a0), "=&v"(a1), "=&v"(t0), "=&v"(t1), "=&v"(u0), "=&v"(u1)
      : "v"(v0), "v"(v1), "v"(c.c0), "v"(c.cm1), "v"(c.cm2), "v"(c.cp1), "v"(c.cp2),
        "v"(d.c0), "v"(d.cm1), "v"(d.cm2), "v"(d.cp1), "v"(d.cp2));
}

// In-place Gauss-Jordan inverse of the 60 x 60 SPD S (one row per lane in and
// out, pivots <= 1 after the 1/max-diagonal scaling): invert_w1's element
// scheme, pivot for pivot and entry for entry, with the rank-1
// update K[i][j] = fma(c_j, ng_i, K[i][j]) of all 64 x 64 entries on the matrix
// cores -- two v_mfma_f32_32x32x1_2b_f32 per pivot instead of 60
// v_fmac_f32_dpp, each entry still one fused multiply-add of the same
// operands, so the same bits (tools/micro/lit_mfma_gj.hip).
//
// Accumulator layout.  The 64 x 64 matrix is four 32 x 32 blocks
// (jb, ib) = (j / 32, i / 32) of (column j, row i); the MFMA's row index is the
// column j and its column index, the lane, the row i.  Register q of block
// (jb, ib) holds, in lane l, K[32 ib + (l & 31)][32 jb + j0(q) + 4 (l / 32)] with
// j0(q) = (q & 3) + 8 (q / 4) (the 32 x 32 C/D map).  D1 carries the blocks
// (0, 0) and (1, 1) -- operands c and ng as they stand --, D2 the blocks (0, 1)
// and (1, 0) -- ng with its lane halves exchanged.  Row registers j0 and
// j0 + 4 of a half jb turn into register q of the blocks (jb, 0) and (jb, 1) by
// one v_permlane32_swap, and back by the same swap: no entry is assumed equal
// to its transpose.  Column k of every row is then one register of each of the
// blocks (jb, 0), (jb, 1), in lane half (k / 4) & 1: one more swap makes it the
// 64-lane vector v, and nothing goes through LDS.
typedef float f32x32 __attribute__((ext_vector_type(32)));
__device__ __forceinline__ void lit_swap32(float &a, float &b) {
  const auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b), false, false);
  // (elements copied out first: __builtin_bit_cast of the vector element r[1]
  // itself reads element 0 with this compiler)
  const unsigned r0 = r[0], r1 = r[1];
  a = __builtin_bit_cast(float, r0);  // (a's lanes < 32, b's lanes < 32)
  b = __builtin_bit_cast(float, r1);  // (a's lanes >= 32, b's lanes >= 32)
}
constexpr int lit_gj_j0(int q) { return (q & 3) + 8 * (q >> 2); }

template <int k>
__device__ __forceinline__ void lit_pivot(f32x32 &D1, f32x32 &D2) {
  constexpr int jb = k >> 5, kk = k & 31, h = (kk >> 2) & 1, q = (kk & 3) + 4 * (kk >> 3);
  static_assert(lit_gj_j0(q) + 4 * h == kk, "column k: register q of the blocks (jb, .), lane half h");
  constexpr int x = jb == 0 ? q : 16 + q;  // block (jb, 0) is D1[x] for jb = 0, D2[x] for jb = 1; block (jb, 1) the other
  // the pivot's lane predicates are constants of k: 64-bit lane masks in SGPRs
  // as the select conditions
  const bool is_k = __builtin_amdgcn_inverse_ballot_w64(1ull << k);
  const bool before_k = __builtin_amdgcn_inverse_ballot_w64((1ull << k) - 1ull);
  const bool lo = __builtin_amdgcn_inverse_ballot_w64(0xffffffffull);
  float X = jb == 0 ? D1[x] : D2[x], Y = jb == 0 ? D2[x] : D1[x];
  lit_swap32(X, Y);
  const float v = h == 0 ? X : Y;  // lane i: K[i][k]
  const float p = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), k));
  const float pinv = __builtin_amdgcn_rcpf(p);
  const float ng = is_k ? pinv - 1.0f : -v * pinv;  // -(1 - pinv), -(v pinv): the same bits, no sign flip after the select
  const float c = is_k ? p + 1.0f : (before_k ? -v : v);  // row k from column k (the symmetric sweep's signs)
  float nl = ng, nh = ng;
  lit_swap32(nl, nh);
  const float ngs = lo ? nh : nl;  // ng with its lane halves exchanged
  D1 = __builtin_amdgcn_mfma_f32_32x32x1f32(c, ng, D1, 0, 0, 0);
  D2 = __builtin_amdgcn_mfma_f32_32x32x1f32(c, ngs, D2, 0, 0, 0);
  if (p > kGjExactPivot) {  // column k exactly: rows < 32 sit in block (jb, 0), rows >= 32 in block (jb, 1), lane half h
    const bool is_ks = __builtin_amdgcn_inverse_ballot_w64(1ull << (k ^ 32));
    const bool half_h = h == 0 ? lo : !lo;
    const float e = is_k ? pinv : ng, es = is_ks ? pinv : ngs;
    const float e0 = h == 0 ? e : es, e1 = h == 0 ? es : e;
    if constexpr (jb == 0) {
      D1[x] = half_h ? e0 : D1[x];
      D2[x] = half_h ? e1 : D2[x];
    } else {
      D2[x] = half_h ? e0 : D2[x];
      D1[x] = half_h ? e1 : D1[x];
    }
  }
}

__device__ __forceinline__ void lit_invert(int ncol, Row<1> &K) {
  int nc = __builtin_amdgcn_readfirstlane(ncol);
  f32x32 D1, D2;
#pragma unroll
  for (int jb = 0; jb < 2; ++jb) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      float a = K.k[32 * jb + lit_gj_j0(q)], b = K.k[32 * jb + lit_gj_j0(q) + 4];
      lit_swap32(a, b);  // a: block (jb, 0), b: block (jb, 1)
      if (jb == 0) {
        D1[q] = a;
        D2[q] = b;
      } else {
        D2[16 + q] = a;
        D1[16 + q] = b;
      }
    }
  }
  ColLoop<0, 60>::run([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    asm volatile("" : "+s"(nc));
    if (k >= nc) return;
    lit_pivot<k>(D1, D2);
  });
#pragma unroll
  for (int jb = 0; jb < 2; ++jb) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      float a = jb == 0 ? D1[q] : D2[16 + q], b = jb == 0 ? D2[q] : D1[16 + q];
      lit_swap32(a, b);
      K.k[32 * jb + lit_gj_j0(q)] = a;
      K.k[32 * jb + lit_gj_j0(q) + 4] = b;
    }
  }
}

// The two-wave form: S is (60 + 60) x (60 + 60) in column space (wave w's
// rows are rows 60 w .. 60 w + 59, its first nc_w valid), one row of 120
// registers per lane.  Each pivot publishes its column (the pivot row up to
// the Gauss-Jordan signs) from both waves into the parity buffer, one
// workgroup barrier, then both halves take the one-wave DPP update.  The
// look-ahead publishes the next pivot's column before the 120-column update,
// so the barrier never waits on that write; the pivot value itself travels
// through LDS (the other wave cannot read the owner's register).
//
// Pivot order: LAST step first (half 1 from its last valid row down, then
// half 0).  S's early steps carry the largest horizon weights (K0 = N - j,
// K2 ~ (N - j)^3 / 3): eliminating them first, as the one-wave kernel's
// natural order does, grows the error of the pivot-free fp32 Gauss-Jordan
// past what ADMM tolerates at N = 16 / 20 and small rho (57 + 4 of 65,536
// N = 16 trot instances ended at max_iter / solved-inaccurate; the float32
// emulation, tools/proto_lit_fused.py, reproduces it and converges with the
// reversed order on every one of them).
template <int HF, int KL>
__device__ __forceinline__ void lit2_pivot(LitLds<2> &S, int wv, int nc, Row<2> &K) {
  const int tt = fresh_lane();
  if constexpr (KL >= 1) {
    if (KL == nc) {  // the half's first pivot (column KL - 1): a plain publish
      constexpr int k1 = 60 * HF + KL - 1;
      const float v = K.k[k1];
      const bool own1 = wv == HF && tt == KL - 1;
      const bool before = HF == 0 && wv == 1;  // half 1 is done when half 0 starts
      reinterpret_cast<float *>(&S.bc[k1 & 1][wv][0])[tt] = own1 ? v + 1.0f : (before ? -v : v);
      if (own1) S.piv[k1 & 1] = v;
    }
  }
  if constexpr (KL < 60) {
    constexpr int k = 60 * HF + KL;
    constexpr int pb = k & 1;
    if (KL >= nc) return;
    bsync<2>();
    const f4v r0 = S.bc[pb][0][tt & 15];
    const f4v r1 = S.bc[pb][1][tt & 15];
    const float p = S.piv[pb];
    const float v = K.k[k];
    const float pinv = __builtin_amdgcn_rcpf(p);
    const bool own = wv == HF && tt == KL;
    const float ng = own ? pinv - 1.0f : -v * pinv;
    if constexpr (KL >= 1) {  // look-ahead: the next pivot is column k - 1 of this half
      const float la = fmaf(dpp_col<KL - 1>(HF ? r1 : r0), ng, K.k[k - 1]);
      const bool own1 = wv == HF && tt == KL - 1;
      const bool before = HF ? (wv == 1 && tt >= KL) : (wv == 1 || tt >= KL);
      reinterpret_cast<float *>(&S.bc[pb ^ 1][wv][0])[tt] = own1 ? la + 1.0f : (before ? -la : la);
      if (own1) S.piv[pb ^ 1] = la;
    }
    QL_DPP_GJ60(K.k, 0, r0, ng);
    QL_DPP_GJ60(K.k, 60, r1, ng);
    if (p > kGjExactPivot) K.k[k] = own ? pinv : ng;
  }
}

__device__ __forceinline__ void lit_invert2(LitLds<2> &S, int wv, int nc0, int nc1, Row<2> &K) {
  nc0 = __builtin_amdgcn_readfirstlane(nc0);
  nc1 = __builtin_amdgcn_readfirstlane(nc1);
  ColLoop<0, 61>::run([&](auto kc) {  // half 1, KL = 60 .. 0
    asm volatile("" : "+s"(nc1));
    lit2_pivot<1, 60 - decltype(kc)::value>(S, wv, nc1, K);
  });
  ColLoop<0, 61>::run([&](auto kc) {  // half 0
    asm volatile("" : "+s"(nc0));
    lit2_pivot<0, 60 - decltype(kc)::value>(S, wv, nc0, K);
  });
  bsync<2>();
}

// Lane-derived indices re-derived from an opaque copy of the lane at the top
// of a phase: the address arithmetic on them is then recomputed there (a few
// VALU) instead of hoisted to the kernel entry and kept live -- at 128 VGPRs
// the hoisted offsets were the setup's scratch spills.  jr / stepl: the
// wave-local step (per-wave LDS rows); step: the global step (the
// gradient, the contact flags, the persistent record); jc: the column-space
// step (the horizon tables: 10 w + jr).  Padding lanes sit on steps whose
// K0 / K2 weights are zero.
#define QL_LIT_LANE_INDICES(LX)                                                                    \
  const int LX = fresh_lane();                                                                     \
  const int jr = LX < 60 ? LX / 6 : kLitN - 1, sr = LX < 60 ? LX - 6 * (LX / 6) : 0;               \
  const int jc = W == 1 ? jr : 10 * wv + jr;                                                       \
  const bool wvalid = LX < nw;                                                                     \
  const int step[2] = {LX < 60 && LX < nvl ? so + LX / 12 : so, LX < 60 && 60 + LX < nvl ? so + (60 + LX) / 12 : so}; \
  const int stepl[2] = {step[0] - so, step[1] - so};                                               \
  const int leg[2] = {LX < 60 && LX < nvl ? (LX % 12) / 3 : 0, LX < 60 && 60 + LX < nvl ? ((60 + LX) % 12) / 3 : 0}; \
  const int comp = LX % 3;                                                                         \
  const bool xy = comp < 2;                                                                        \
  const bool valid[2] = {LX < 60 && LX < nvl, LX < 60 && 60 + LX < nvl};                           \
  (void)jr; (void)sr; (void)jc; (void)wvalid; (void)stepl; (void)step; (void)leg; (void)comp; (void)xy; (void)valid

// WS: a warm-start mode (1 or 2) may be set (the persistent record of
// DESIGN.md §3c, literal semantics: the update path on every call).
// MR: the call carries model rows (a.model); false compiles to the code of a
// kernel that knows no rows.
template <int W, bool WS, bool MR>
__device__ __forceinline__ void srbd_lit_one(const SrbdArgs &a, LitLds<W> &S, const int64_t b) {
  constexpr int NS = LitLds<W>::NS, NT = LitLds<W>::NT;
  const int lane = W == 1 ? (int)threadIdx.x : (int)(threadIdx.x & 63);
  const int tid = threadIdx.x;
  const int wv = W == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int N = a.N;
  const float Nf = (float)N;
  const float dt = a.dt;
  // with rows, a phase loads the values it needs again (an opaque index: the
  // loads are not merged with the first ones and held in SGPRs across the
  // setup -- the one-wave kernel has none to spare)
  SrbdBodyAt<MR> body{a};
  auto load_body = [&] {
    if constexpr (MR) {
      int64_t bb = b;
      asm volatile("" : "+s"(bb));
      body.row = srbd_body(a, bb);
    }
  };
  if constexpr (MR) {
    body.row = srbd_body(a, b);
    if (srbd_body_bad(body.row)) {  // uniform, before the first barrier and the first write
      // (a thread index of its own: none is kept for it across the solve)
      srbd_refuse<64 * W>(a, b, W == 1 ? fresh_lane() : opaque_tid(), QLOCO_ERR_ARG);
      return;
    }
  }
  const float dtm = dt / body.mass(), dt2m = dt * dt / body.mass();
  // this wave's steps: [so, so + Nw) (W = 1: all N)
  const int H = W == 1 ? N : (N + 1) / 2;
  const int so = W == 1 ? 0 : wv * H;
  const int Nw = W == 1 ? N : (wv ? N - H : H);
  const int nvar = 12 * N, nvl = 12 * Nw, nw = 6 * Nw;

  // ---------------- 1. inputs -> LDS
  if (tid < 13) S.x0[tid] = a.x0[b * 13 + tid];
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 13; ++k) S.q2[k] = a.q2[k];
#pragma unroll
    for (int k = 0; k < 12; ++k) S.r2[k] = a.r2[k];
  }
  {
    const int nct = a.contacts_per_step ? 4 * N : 4;
    if (tid < 4 * N) S.ctf[tid] = a.contacts[b * nct + (a.contacts_per_step ? tid : (tid & 3))] ? 1.0f : 0.0f;
  }
  for (int idx = tid; idx < NT * NT; idx += 64 * W) {
    const int sr = idx / NT, sc = idx - NT * sr;
    float K0 = 0.0f, K2 = 0.0f;
    if constexpr (W == 1) {
      if (sr < N && sc < N) k0k2((float)sr, (float)sc, Nf, K0, K2);
    } else {  // column-space steps -> global steps (-1: padding)
      const int gr = sr % 10 < (sr >= 10 ? N - H : H) ? (sr >= 10 ? H : 0) + sr % 10 : -1;
      const int gc = sc % 10 < (sc >= 10 ? N - H : H) ? (sc >= 10 ? H : 0) + sc % 10 : -1;
      if (gr >= 0 && gc >= 0) k0k2((float)gr, (float)gc, Nf, K0, K2);
    }
    S.k0k2[sr][sc] = (f2v){K0, K2};
  }
  if constexpr (W == 2) {  // Ruiz column scales of the padding steps stay 0
    for (int idx = tid; idx < 12 * NT; idx += 64 * W) S.dcol[idx] = 0.0f;
  }
  bsync<W>();

  // ---------------- 2. SRBD model (ConvexMpc.cpp:111-160, compute_grf :502-549)
  const float yaw = S.x0[2];
  float sy, cy;
  sincosf(yaw, &sy, &cy);  // one range reduction; the bits of sinf / cosf
  const float R00 = cy, R01 = sy, R10 = -sy, R11 = cy;  // A1RobotControl.cpp:506-508
  if constexpr (W == 1) {
    // host G^-1 tables (isotropic omega weights): the omega
    // x / y pair's S = Q^-1/2 V with V = Rz' -- the eigenvectors of
    // Rz' diag(q_theta) Rz / q_omega for every yaw -- from the model's cos / sin
    if (a.lit_tables && tid == 0) {
      const float sq = a.lit_sq;
      S.sc[0].sxy[0][0] = sq * cy;
      S.sc[0].sxy[0][1] = -(sq * sy);
      S.sc[0].sxy[1][0] = sq * sy;
      S.sc[0].sxy[1][1] = sq * cy;
    }
  }
  float Ii[3][3];
  srbd_inertia_inv(cy, sy, body.inertia(), Ii);
  // per slot: the variable, its B_d column (omega rows: ba) and E column
  const int comp = lane % 3;
  const bool xy = comp < 2;
  bool valid[2];
  int step[2], leg[2], cst[2];  // global / column-space step
  f4v lo[2], hi[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int v = 60 * h + lane;
    valid[h] = lane < 60 && v < nvl;
    step[h] = valid[h] ? so + v / 12 : 0;
    cst[h] = W == 1 ? step[h] : (valid[h] ? 10 * wv + v / 12 : 0);
    leg[h] = valid[h] ? (v % 12) / 3 : 0;
    float ba[3];  // constant feet only (srbd_route_of)
    srbd_bd_column(Ii, srbd_foot(a.feet, b, N, 0, step[h], leg[h]), comp, dt, R00, R01, R10, R11,
                   step[h], valid[h], ba, lo[h], hi[h]);
    // the wrench map (constant feet): column v % 12 of Bb from the step-0 lanes
    if (h == 0 && tid < 12) {
      S.Bb[0][lane] = ba[0];
      S.Bb[1][lane] = ba[1];
      S.Bb[2][lane] = ba[2];
      S.Bb[3][lane] = comp == 0 ? dtm : 0.0f;
      S.Bb[4][lane] = comp == 1 ? dtm : 0.0f;
      S.Bb[5][lane] = comp == 2 ? dtm : 0.0f;
    }
  }
  // Te = dt^2 blockdiag(Rz' diag(q2[0:3]) Rz, diag(q2[3:6]))
  if (tid < 36) {
    const int r = lane / 6, c = lane - 6 * (lane / 6);
    const float Rm[3][3] = {{R00, R01, 0.f}, {R10, R11, 0.f}, {0.f, 0.f, 1.f}};
    float v = 0.0f;
    if (r < 3 && c < 3)
      v = dt * dt * (Rm[0][r] * S.q2[0] * Rm[0][c] + Rm[1][r] * S.q2[1] * Rm[1][c] + Rm[2][r] * S.q2[2] * Rm[2][c]);
    else if (r >= 3 && c == r)
      v = dt * dt * S.q2[r];
    S.Te[r][c] = v;
  }
  float r2v[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) r2v[h] = valid[h] ? S.r2[3 * leg[h] + comp] : 0.0f;

  // ---------------- 3. gradient g = Bqp' Q (Aqp x0 - x_ref) (ConvexMpc.cpp:219-221)
  for (int idx = tid; idx < 12 * N; idx += 64 * W) {
    const int i = idx / 12, s = idx - 12 * i;
    const float xf = srbd_free_state<12>(S.x0, s, i, dt, R00, R01, R10, R11);
    S.err[idx] = S.q2[s] * (xf - a.xref[b * 13 * N + 13 * i + s]);
  }
  bsync<W>();
  if (tid < 12) {  // suffix scans per state row (row_scans of the two-wave kernel)
    const int r = lane;
    const bool brow = r >= 6;
    float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
    for (int j = NS - 1; j >= 0; --j) {
      if (j < N) {
        s1 += s0;
        s0 += S.err[12 * j + r];
        S.Wc[12 * j + r] = brow ? s0 : s1;
      }
    }
  }
  bsync<W>();
  float qv[2], qsv[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    float g = 0.0f;
    if (valid[h]) {
      const float *w = S.Wc + 12 * step[h];
      g = lo[h].x * w[6] + lo[h].y * w[7] + lo[h].z * w[8];
      g += lo[h].w * w[0] + hi[h].x * w[1] + hi[h].y * w[2];
      g += dtm * w[9 + comp] + dt2m * w[3 + comp];
    }
    qv[h] = g;
    qsv[h] = g;
  }
  // from here on a variable's B_d column is all the iterations need of lo/hi:
  // its omega rows (the wrench map's torque part; the force part is dtm e_comp)
  // persistent solver (warm_start == 2): literal semantics -- after the
  // first call every call takes OSQP's update path
  const int NP = 100 * N;
  float *prec = (WS && a.warm_start == 2) ? a.warm + b * (int64_t)(NP + 4) : nullptr;
  bool p_init = false;
  if (prec) p_init = prec[NP + 1] > 0.5f;
  const bool p_same = p_init;
  if (p_same) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
      if (valid[h]) qsv[h] = prec[84 * N + 12 * step[h] + 3 * leg[h] + comp];
  }
  if (prec) {  // the record's q for the next call, written now (each variable's own entry, just read)
#pragma unroll
    for (int h = 0; h < 2; ++h)
      if (valid[h]) prec[84 * N + 12 * step[h] + 3 * leg[h] + comp] = qv[h];
  }

  // ---------------- 4. constraint rows owned by each slot (ConvexMpc.cpp:47-59, :227-249)
  float ra0[2], ra1[2], rz0[2], rz1[2], rl0[2], ru0[2];
  load_body();
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    ra0[h] = valid[h] ? 1.0f : 0.0f;
    ra1[h] = (valid[h] && xy) ? 1.0f : 0.0f;
    rz0[h] = (valid[h] && xy) ? body.mu() : 0.0f;
    rz1[h] = (valid[h] && xy) ? -body.mu() : 0.0f;
    const float cflag = valid[h] ? S.ctf[4 * step[h] + leg[h]] : 0.0f;
    rl0[h] = !valid[h] ? 0.0f : (xy ? 0.0f : body.fz_min() * cflag);
    ru0[h] = !valid[h] ? 0.0f : (xy ? INFINITY : body.fz_max() * cflag);
  }

  // ---------------- 5. modified Ruiz equilibration (OSQP scaling.c), P rows
  // generated from the wrench structure: P[(j,w),(k,w')] = K0(j,k) beta[w][w']
  // + K2(j,k) eps[w][w'] + R delta, beta = <b_w, b_w'>_Qb, eps = <b_w, b_w'>_Te
  float rE0[2] = {1.0f, 1.0f}, rE1[2] = {1.0f, 1.0f}, Dr[2] = {1.0f, 1.0f}, cs = 1.0f;
  {
    // beta / eps tables (12 x 12, constant feet) in LDS: beta[w][w'] =
    // sum_s Qb_s Bb[s][w] Bb[s][w'], eps[w][w'] = Bb[:,w]' Te Bb[:,w']
    bsync<W>();
    for (int e = tid; e < 144; e += 64 * W) {
      const int w = e / 12, wp = e - 12 * (e / 12);
      float bb = 0.0f, ee = 0.0f;
#pragma unroll
      for (int s = 0; s < 6; ++s) {
        bb = fmaf(S.q2[6 + s] * S.Bb[s][w], S.Bb[s][wp], bb);
        float tw = 0.0f;
#pragma unroll
        for (int t = 0; t < 6; ++t) tw = fmaf(S.Te[s][t], S.Bb[t][wp], tw);
        ee = fmaf(S.Bb[s][w], tw, ee);
      }
      S.beps[w][wp] = (f2v){bb, ee};
    }
    bsync<W>();
    // this lane's diagonal P entries (R included)
    float pdiag[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int wl = valid[h] ? (60 * h + lane) % 12 : 0;
      const f2v kk = S.k0k2[cst[h]][cst[h]];
      const f2v be = S.beps[wl][wl];
      pdiag[h] = valid[h] ? fmaf(kk.y, be.y, kk.x * be.x) + r2v[h] : 0.0f;
    }
    // this lane's (beta, eps) row as pairs of adjacent columns (w, w + 1),
    // registers for the whole of Ruiz.  Both slots of a lane sit on the same
    // wrench column (60 % 12 == 0), so one row serves both: 24 registers, and
    // the pairs {beta_w, beta_w+1}, {eps_w, eps_w+1} and {D_w, D_w+1} (as
    // read) are the packed operands as they stand -- no pair-building moves
    // (DESIGN.md §3l).  A slot that holds no variable computes on the lane's
    // row all the same and is masked at the end.
    f2v be2[6], ep2[6];
    {
      const int wl = lane < 60 ? lane % 12 : 0;
#pragma unroll
      for (int p = 0; p < 6; ++p) {
        const f4v q = *reinterpret_cast<const f4v *>(&S.beps[wl][2 * p]);  // (beta, eps) of w, w + 1
        be2[p] = (f2v){q.x, q.z};
        ep2[p] = (f2v){q.y, q.w};
      }
    }
    // row inf-norms |P_vc| D_c of both slots' rows in one sweep over the 12N
    // columns, step-major: per column step the K0 / K2 weights of the two
    // rows' steps and the step's 12 column scales (same-address LDS reads,
    // a broadcast), then 12 entries per row from the (beta, eps) row: every
    // entry fma(K2, eps, K0 beta) D, whatever the packing
    auto row_norms = [&](bool scaled, float (&m)[2]) {
      // loop-invariant tables: opaque per call (no hoisting of all 240 entries)
#pragma unroll
      for (int p = 0; p < 6; ++p) asm volatile("" : "+v"(be2[p]), "+v"(ep2[p]));
      // column pairs as fp32 pairs (v_pk_fma / v_pk_mul, K0 / K2 broadcast
      // from the pair as loaded), two max chains per slot; the next column
      // step's LDS reads are issued before this step's arithmetic (one step
      // of look-ahead, no more: all ten would be live)
      float ma[2] = {0.0f, 0.0f}, mb[2] = {0.0f, 0.0f};
      const f4v one4 = (f4v)(1.0f);
      f2v k0 = S.k0k2[cst[0]][0], k1 = S.k0k2[cst[1]][0];
      f4v da = scaled ? reinterpret_cast<const f4v *>(&S.dcol[0])[0] : one4,
          db = scaled ? reinterpret_cast<const f4v *>(&S.dcol[0])[1] : one4,
          dd = scaled ? reinterpret_cast<const f4v *>(&S.dcol[0])[2] : one4;
#pragma unroll
      for (int kc = 0; kc < NS; ++kc) {
        const int kn = kc + 1 < NS ? kc + 1 : kc;
        asm volatile("" ::: "memory");  // table reads stay in the pass (no LICM)
        const f2v k0n = S.k0k2[cst[0]][kn], k1n = S.k0k2[cst[1]][kn];
        const f4v *dcn = reinterpret_cast<const f4v *>(&S.dcol[12 * kn]);
        const f4v dan = scaled ? dcn[0] : one4, dbn = scaled ? dcn[1] : one4, ddn = scaled ? dcn[2] : one4;
        __builtin_amdgcn_sched_barrier(0);
        const f2v dv[6] = {{da.x, da.y}, {da.z, da.w}, {db.x, db.y}, {db.z, db.w}, {dd.x, dd.y}, {dd.z, dd.w}};
        // four independent chains at a time (slot c >> 1, column pair
        // 2 g + (c & 1)), stage by stage: a packed op's result is read three
        // instructions later, so no hazard padding between dependent ops
#pragma unroll
        for (int g = 0; g < 3; ++g) {
          f2v t[4];
#pragma unroll
          for (int c = 0; c < 4; ++c) t[c] = (f2v)((c >> 1) ? k1.x : k0.x) * be2[2 * g + (c & 1)];
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int c = 0; c < 4; ++c)
            t[c] = __builtin_elementwise_fma((f2v)((c >> 1) ? k1.y : k0.y), ep2[2 * g + (c & 1)], t[c]);
          __builtin_amdgcn_sched_barrier(0);
          if (scaled) {
#pragma unroll
            for (int c = 0; c < 4; ++c) t[c] = t[c] * dv[2 * g + (c & 1)];
            __builtin_amdgcn_sched_barrier(0);
          }
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            float &acc = (c & 1) ? mb[c >> 1] : ma[c >> 1];
            acc = fmaxf(fmaxf(acc, fabsf(t[c].x)), fabsf(t[c].y));
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        // pin the step's arithmetic here (no sinking into a late masked block
        // that would keep every step's loads live)
        asm volatile("" : "+v"(ma[0]), "+v"(ma[1]), "+v"(mb[0]), "+v"(mb[1]));
        __builtin_amdgcn_sched_barrier(0);
        k0 = k0n;
        k1 = k1n;
        da = dan;
        db = dbn;
        dd = ddn;
      }
      m[0] = valid[0] ? fmaxf(ma[0], mb[0]) : 0.0f;
      m[1] = valid[1] ? fmaxf(ma[1], mb[1]) : 0.0f;
    };
    float cnP[2];
    {
      float m[2];
      row_norms(false, m);
#pragma unroll
      for (int h = 0; h < 2; ++h) cnP[h] = valid[h] ? fmaxf(m[h], pdiag[h]) : 0.0f;
    }
    const float inv_n = 1.0f / (float)nvar;
    for (int it = 0; it < a.scaling; ++it) {
      float Dt[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float cnA = fmaxf(fabsf(ra0[h]), fabsf(ra1[h]));
        const float zmax = fmaxf(fabsf(rz0[h]), fabsf(rz1[h]));
        const float zm1 = lane_prev(zmax), zm2 = lane_prev(zm1);
        if (comp == 2) cnA = fmaxf(cnA, fmaxf(zm1, zm2));
        Dt[h] = valid[h] ? __builtin_amdgcn_rsqf(limit_scaling(fmaxf(cnP[h], cnA))) : 1.0f;
        const float Et0 = valid[h] ? __builtin_amdgcn_rsqf(limit_scaling(fmaxf(fabsf(ra0[h]), fabsf(rz0[h])))) : 1.0f;
        const float Et1 = (valid[h] && xy) ? __builtin_amdgcn_rsqf(limit_scaling(fmaxf(fabsf(ra1[h]), fabsf(rz1[h])))) : 1.0f;
        const float Dn1 = lane_next(Dt[h]), Dn2 = lane_next(Dn1);
        const float Dz = comp == 0 ? Dn2 : (comp == 1 ? Dn1 : Dt[h]);
        ra0[h] *= Et0 * Dt[h];
        ra1[h] *= Et1 * Dt[h];
        rz0[h] *= Et0 * Dz;
        rz1[h] *= Et1 * Dz;
        rE0[h] *= Et0;
        rE1[h] *= Et1;
        qv[h] *= Dt[h];
        qsv[h] *= Dt[h];
        Dr[h] *= Dt[h];
        if constexpr (W == 1) {
          if (lane < 60) S.dcol[60 * h + lane] = valid[h] ? Dr[h] : 0.0f;
        } else {
          if (valid[h]) S.dcol[120 * wv + 60 * h + lane] = Dr[h];  // column-space order
        }
      }
      bsync<W>();
      float cn2[2], mr[2];
      row_norms(true, mr);
#pragma unroll
      for (int h = 0; h < 2; ++h) cn2[h] = valid[h] ? Dr[h] * fmaxf(mr[h], pdiag[h] * Dr[h]) : 0.0f;
      // cost scaling: mean column norm of the scaled P vs ||q||_inf
      const float sumP = bsum<W>(S, wsum(cn2[0] + cn2[1]), wv);
      const float qm = bmax1<W>(S, wmax_nonneg(fmaxf(valid[0] ? fabsf(qsv[0]) : 0.0f, valid[1] ? fabsf(qsv[1]) : 0.0f)), wv);
      const float meanP = cs * sumP * inv_n;
      const float ctc = __builtin_amdgcn_rcpf(limit_scaling(fmaxf(meanP, limit_scaling(qm))));
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        qv[h] *= ctc;
        qsv[h] *= ctc;
        cnP[h] = cn2[h] * cs * ctc;
      }
      cs *= ctc;
      bsync<W>();
    }
  }
  // block-uniform scalars live in SGPRs (a VGPR copy would be kept, and
  // spilled, across the whole ADMM loop)
  cs = sgpr_f(cs);
  const float cinv0 = sgpr_f(1.0f / cs);
  bool eq0[2];
  float qn[2] = {0.0f, 0.0f};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float lh0 = rl0[h] * rE0[h], uh0 = ru0[h] * rE0[h];
    eq0[h] = valid[h] && !xy && (uh0 - lh0 < 1e-4f);  // OSQP set_rho_vec: RHO_TOL
    S.zh[wv][h][lane] = uh0;
    S.dr[wv][h][lane] = Dr[h];
    S.qvl[wv][h][lane] = qv[h];
    S.arz[wv][h][lane] = (f4v){ra0[h], ra1[h], rz0[h], rz1[h]};
    qn[0] = fmaxf(qn[0], valid[h] ? fabsf(qv[h] / Dr[h]) : 0.0f);
    qn[1] = fmaxf(qn[1], valid[h] ? fabsf(qv[h]) : 0.0f);
  }
  qn[0] = wmax_nonneg(qn[0]);
  qn[1] = wmax_nonneg(qn[1]);
  bcombine_max<W, 2>(S, qn, wv);
  S.sc[wv].cs = cs;  // every lane the same value
  S.sc[wv].cinv = cinv0;
  S.sc[wv].qn0 = qn[0];
  S.sc[wv].qn1 = qn[1];
  lsync();

  // row scaling E of a slot's two rows, from A~ = E A D (each row's entry in
  // its own variable's column is 1 before scaling)
  auto row_e = [&](int h) -> f2v {
    const int fl = fresh_lane();
    const f4v arz = S.arz[wv][h][fl];
    const float d = S.dr[wv][h][fl];
    return (f2v){valid[h] ? arz.x / d : 1.0f, (valid[h] && xy) ? arz.y / d : 1.0f};
  };

  // wrench row of this lane: step jr, component sr; its row of Bb (12)
  const bool wvalid = lane < nw;
  // lanes 6N..59 carry the (identity) factors of the padding steps, whose
  // K0 / K2 weights are zero; lanes 60..63 only pad
  const int jr = lane < 60 ? lane / 6 : kLitN - 1, sr = lane < 60 ? lane - 6 * (lane / 6) : 0;
  // this lane's row of Bb (12) is read from LDS where used (registers are
  // the factorisation's bound); padding wrench lanes get zeros
  // through their K0 / K2 weights and masks
  // this lane's variables' wrench columns (omega rows = lo.xyz, v row = dtm at comp)
  S.sc[wv].rho = sgpr_f(fminf(fmaxf(p_same ? prec[NP] : a.rho, 1e-6f), 1e6f));

  // ---------------- 6. ADMM (osqp_solve) with its (re)factorisations
  float x[2] = {0.0f, 0.0f};
  f2v z[2] = {(f2v)(0.0f), (f2v)(0.0f)}, y[2] = {(f2v)(0.0f), (f2v)(0.0f)};
  {
    S.sc[wv].alpha = a.alpha;
    S.sc[wv].oma = 1.0f - a.alpha;
    S.sc[wv].sigma = a.sigma;
    S.sc[wv].dtm = dtm;
    load_body();
    S.sc[wv].zlo = body.fz_max() > 0.0f ? body.fz_min() / body.fz_max() : 0.0f;
    const int ctm = a.check_termination;
    S.sc[wv].ctm = ctm;
    S.sc[wv].interval = (a.adaptive_rho && a.rho_interval == 0) ? (ctm ? 4 * ctm : 100)
                                                                : (a.adaptive_rho ? a.rho_interval : 0);
    S.sc[wv].iter = 0;
    S.sc[wv].status = QLOCO_MAX_ITER;
    S.sc[wv].rho_updates = 0;
  }
  lsync();
  auto uf = [&](const float &v) { return sgpr_f(v); };  // an LDS scalar into an SGPR
  auto ui = [&](const int &v) { return __builtin_amdgcn_readfirstlane(v); };
  Row<W> T;        // T = (I + cG U)^-1 cG, this lane's wrench row (column space)
  Shift5 W1[2];  // per slot: this lane's row of W0^-1 as leg-triple shifts

  // P~ x (scaled) per slot: c D (Vu' G Vu + R) D x through the wrench rows
  auto p_times_x = [&](float (&out)[2]) {
    if constexpr (W == 2) bsync<W>();  // the other wave is done with the iteration's broadcast rows
    QL_LIT_LANE_INDICES(lxp);
    const float drp[2] = {S.dr[wv][0][lxp], S.dr[wv][1][lxp]};
    const float csl = uf(S.sc[wv].cs), dtm = uf(S.sc[wv].dtm);
#pragma unroll
    for (int h = 0; h < 2; ++h) S.av[wv][h][lxp] = valid[h] ? x[h] * drp[h] : 0.0f;
    lsync();
    // w = Vu (D x): wrench row (jr, sr) sums its step's 12 variables
    float wr = 0.0f;
    {
      const int hh = jr >= 5 ? 1 : 0, base = 12 * (jr - 5 * hh);
      const f4v *src = reinterpret_cast<const f4v *>(&S.av[wv][hh][base]);
      const f4v u0 = src[0], u1 = src[1], u2 = src[2];
      const float uv[12] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w, u2.x, u2.y, u2.z, u2.w};
      const f4v *br = reinterpret_cast<const f4v *>(S.Bb[sr]);
      const f4v b0 = br[0], b1 = br[1], b2 = br[2];
      const float bv[12] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w, b2.x, b2.y, b2.z, b2.w};
#pragma unroll
      for (int w = 0; w < 12; ++w) wr = fmaf(bv[w], uv[w], wr);
      wr = wvalid ? wr : 0.0f;
    }
    S.wv[wv][lxp] = wr;
    lsync();
    // Te w per row (needs the step's 6 wrench values)
    {
      float tw = 0.0f;
#pragma unroll
      for (int t = 0; t < 6; ++t) tw = fmaf(S.Te[sr][t], S.wv[wv][6 * jr + t], tw);
      reinterpret_cast<float *>(&S.bc[0][wv][0])[lxp] = wvalid ? tw : 0.0f;  // Te w (bc is free in a check)
    }
    bsync<W>();
    // (G w)[(jr, sr)] = Qb_s sum_k K0(jr,k) w(k,sr) + sum_k K2(jr,k) (Te w_k)_sr
    float gw = 0.0f;
    {
      const float qb = S.q2[6 + sr];
      float s0 = 0.0f, s2 = 0.0f;
#pragma unroll
      for (int wp = 0; wp < W; ++wp) {
#pragma unroll
        for (int k = 0; k < kLitN; ++k) {
          const f2v kk = S.k0k2[jc][10 * wp + k];
          s0 = fmaf(kk.x, S.wv[wp][6 * k + sr], s0);
          s2 = fmaf(kk.y, reinterpret_cast<const float *>(&S.bc[0][wp][0])[6 * k + sr], s2);
        }
      }
      gw = wvalid ? fmaf(qb, s0, s2) : 0.0f;
    }
    bsync<W>();
    S.wv[wv][lxp] = gw;
    lsync();
    // Vu' (G w) + R (D x), then c D (...)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float acc = 0.0f;
      if (valid[h]) {
        const float *gs = &S.wv[wv][6 * stepl[h]];
        const int wc = lxp % 12;  // the variable's column of Bb (both slots: 60 = 5 x 12)
        acc = S.Bb[0][wc] * gs[0] + S.Bb[1][wc] * gs[1] + S.Bb[2][wc] * gs[2] + dtm * gs[3 + comp];
        acc = fmaf(S.r2[3 * leg[h] + comp], x[h] * drp[h], acc);  // valid slot: r2 of its leg
      }
      out[h] = csl * drp[h] * acc;
    }
    lsync();
  };

  auto residuals = [&](float (&o)[6], float (&r)[6], bool want_r) {
    float px[2];
    p_times_x(px);
    QL_LIT_LANE_INDICES(lxr);
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = r[k] = 0.0f;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float Drl = S.dr[wv][h][lxr];
      const float Dinvl = __builtin_amdgcn_rcpf(Drl);
      const f4v arz = S.arz[wv][h][lxr];
      // E^-1 of the slot's rows from A~ = E A D (unit own-column entries)
      const f2v Einv = {valid[h] ? Drl * __builtin_amdgcn_rcpf(arz.x) : 1.0f,
                        (valid[h] && xy) ? Drl * __builtin_amdgcn_rcpf(arz.y) : 1.0f};
      const f2v ra = {arz.x, arz.y}, rz = {arz.z, arz.w};
      const float n1 = lane_next(x[h]), n2 = lane_next(n1);
      const float xz = comp == 0 ? n2 : (comp == 1 ? n1 : x[h]);
      const f2v ay = ra * y[h], az = rz * y[h];
      const float ay_z = az.x + az.y;
      const float p1 = lane_prev(ay_z), p2 = lane_prev(p1);
      const float aty = valid[h] ? ((ay.x + ay.y) + (comp == 2 ? (p1 + p2) : 0.0f)) : 0.0f;
      const float rd = valid[h] ? (S.qvl[wv][h][lxr] + px[h] + aty) : 0.0f;
      const f2v ax = ra * x[h] + rz * xz;
      const f2v rp = ax - z[h];
      const f2v erp = Einv * rp, ez = Einv * z[h], eax = Einv * ax;
      o[0] = fmaxf(o[0], fmaxf(fabsf(erp.x), fabsf(erp.y)));
      o[1] = fmaxf(o[1], fmaxf(fabsf(ez.x), fabsf(ez.y)));
      o[2] = fmaxf(o[2], fmaxf(fabsf(eax.x), fabsf(eax.y)));
      o[3] = fmaxf(o[3], fabsf(Dinvl * rd));
      o[4] = fmaxf(o[4], fabsf(Dinvl * aty));
      o[5] = fmaxf(o[5], fabsf(Dinvl * px[h]));
      if (want_r) {
        r[0] = fmaxf(r[0], fmaxf(fabsf(rp.x), fabsf(rp.y)));
        r[1] = fmaxf(r[1], fmaxf(fabsf(z[h].x), fabsf(z[h].y)));
        r[2] = fmaxf(r[2], fmaxf(fabsf(ax.x), fabsf(ax.y)));
        r[3] = fmaxf(r[3], fabsf(rd));
        r[4] = fmaxf(r[4], fabsf(aty));
        r[5] = fmaxf(r[5], fabsf(px[h]));
      }
    }
    wmax_nonneg6(o);
    if (want_r) wmax_nonneg6(r);
    if constexpr (W == 2) {  // block maxima (r only where the rho estimate needs them)
      float v[12];
#pragma unroll
      for (int k = 0; k < 6; ++k) v[k] = o[k], v[6 + k] = want_r ? r[k] : 0.0f;
      bcombine_max<W, 12>(S, v, wv);
#pragma unroll
      for (int k = 0; k < 6; ++k) o[k] = v[k], r[k] = v[6 + k];
    }
  };

  // warm start (x, z, y) before the first factorisation
  if (WS) {
    QL_LIT_LANE_INDICES(lxs);  // record addresses derived here, not shared with the write-back
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int vidx = 12 * step[h] + 3 * leg[h] + comp, rbase = 20 * step[h] + 5 * leg[h] + 2 * comp;
      if (p_same) {
        x[h] = valid[h] ? prec[vidx] : 0.0f;
        z[h].x = valid[h] ? prec[12 * N + rbase] : 0.0f;
        z[h].y = (valid[h] && xy) ? prec[12 * N + rbase + 1] : 0.0f;
        y[h].x = valid[h] ? prec[32 * N + rbase] : 0.0f;
        y[h].y = (valid[h] && xy) ? prec[32 * N + rbase + 1] : 0.0f;
      } else if (a.warm_start == 1) {
        const float *wx = a.warm + b * (32 * N);
        const float *wy = wx + 12 * N;
        x[h] = valid[h] ? wx[vidx] / S.dr[wv][h][lxs] : 0.0f;
        const f2v e = row_e(h);
        const float csl = uf(S.sc[wv].cs);
        y[h].x = valid[h] ? wy[rbase] / e.x * csl : 0.0f;
        y[h].y = (valid[h] && xy) ? wy[rbase + 1] / e.y * csl : 0.0f;
        const float n1 = lane_next(x[h]), n2 = lane_next(n1);
        const float xz = comp == 0 ? n2 : (comp == 1 ? n1 : x[h]);
        const f4v arz = S.arz[wv][h][lxs];
        z[h] = (f2v){arz.x, arz.y} * x[h] + (f2v){arz.z, arz.w} * xz;
      }
    }
  }
  // G^-1 in six N x N blocks.  G = K0 (x) Qb + K2 (x) Te
  // (Qb = diag(q_omega, q_v), Te = dt^2 blockdiag(Rz' diag(q_theta) Rz,
  // diag(q_p))) splits by wrench component: each v axis and omega_z alone
  // (A_a = alpha_a K0 + beta_a K2), omega_x / omega_y together:
  // G_xy = K0 (x) Q + K2 (x) dt^2 T, Q = diag(q_omega_x, q_omega_y),
  // T = [Rz' diag(q_theta) Rz]_xy.  The 2 x 2 pair (T, Q) is diagonalised
  // together -- S' Q S = I, S' T S = diag(lambda) with S = Q^-1/2 V, V the
  // eigenvectors of Q^-1/2 T Q^-1/2 (one Jacobi rotation) -- so
  // G_xy^-1 = (I (x) S) diag_a (K0 + dt^2 lambda_a K2)^-1 (I (x) S'): two more
  // N x N inverses, recombined through S in the factorisation.  Any omega
  // weights work (q_omega_x != q_omega_y couples the axes: the reference's
  // isaac_a1_mpc.yaml); with q_omega_x = q_omega_y S is Rz' / sqrt(q_omega).
  // One N x N Gauss-Jordan per (axis, row) lane in float64, once per solve,
  // instead of a 6N x 6N one per factorisation.
  //
  // Isotropic omega weights (q_omega_x = q_omega_y: Go1's default set, the
  // reference's gazebo and hardware sets): lambda = (q_theta_x, q_theta_y) /
  // q_omega for every yaw, so all six blocks depend on the spec alone and
  // come from the host with the kernel arguments (one wave: 600 floats;
  // qloco_srbd_tables.cpp); S was stored with the model.
  float gmx = 0.0f;  // max diag G^-1 (block-uniform; an SPD matrix's largest entry)
  bool host_tables = false;  // wave-uniform
  if constexpr (W == 1) host_tables = a.lit_tables != 0;
  if (host_tables) {
    if constexpr (W == 1) {
      static_assert(sizeof(S.gtab) == sizeof(a.lit_gtab) && offsetof(LitLds<1>, gtab) % 16 == 0 &&
                        offsetof(SrbdArgs, lit_gtab) % 16 == 0,
                    "the host tables are copied as f4v into gtab");
      constexpr int NV = (int)(sizeof(a.lit_gtab) / (sizeof(float) * 4));
      const int fl = fresh_lane();
      // read through the kernarg segment itself (SrbdArgs is the kernel's one
      // parameter): a lane-indexed read of the by-value copy would put the
      // whole argument block into scratch
      typedef const f4v __attribute__((address_space(4))) *KernargF4;
      typedef const char __attribute__((address_space(4))) *KernargBytes;
      const KernargBytes args = (KernargBytes)__builtin_amdgcn_kernarg_segment_ptr();
      const KernargF4 src = (KernargF4)(args + offsetof(SrbdArgs, lit_gtab));
      f4v *dst = reinterpret_cast<f4v *>(&S.gtab[0][0][0]);
#pragma unroll
      for (int i = 0; i < (NV + 63) / 64; ++i)
        if (64 * i + fl < NV) dst[64 * i + fl] = src[64 * i + fl];
      gmx = sgpr_f(a.lit_gmx);
      bsync<W>();
    }
  } else {
    double row[NS];
    const int r = tid;
    const bool live = r < 6 * N;
    const int ax = live ? r / N : 0, ri = live ? r - N * (r / N) : 0;
    double sxy[2][2], sn2 = 1.0;  // S; sn2: this lane's axis' S column norm^2 (the gmx bound)
    {
      const double dt2 = (double)dt * (double)dt;
      double lam[2];
      {
        const double qx = (double)S.q2[6], qy = (double)S.q2[7];
        const double yw = (double)S.x0[2], cw = cos(yw), sw = sin(yw);
        const double Rm[2][2] = {{cw, sw}, {-sw, cw}};  // Rz (A1RobotControl.cpp:506-508)
        double T[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            T[i][j] = Rm[0][i] * (double)S.q2[0] * Rm[0][j] + Rm[1][i] * (double)S.q2[1] * Rm[1][j];
        const double ix = 1.0 / sqrt(qx), iy = 1.0 / sqrt(qy);
        const double c00 = T[0][0] * ix * ix, c01 = T[0][1] * ix * iy, c11 = T[1][1] * iy * iy;
        double t = 0.0;  // one Jacobi rotation: tan of the angle that diagonalises C
        if (c01 != 0.0) {
          const double tau = (c11 - c00) / (2.0 * c01);
          t = tau == 0.0 ? 1.0 : (tau > 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
        }
        const double cs = 1.0 / sqrt(1.0 + t * t), sn = t * cs;
        lam[0] = c00 - t * c01;
        lam[1] = c11 + t * c01;
        sxy[0][0] = ix * cs;  // S = Q^-1/2 V, V = [[cs, sn], [-sn, cs]]
        sxy[0][1] = ix * sn;
        sxy[1][0] = -iy * sn;
        sxy[1][1] = iy * cs;
        if (ax < 2) sn2 = sxy[0][ax] * sxy[0][ax] + sxy[1][ax] * sxy[1][ax];
      }
      const double al = ax < 2 ? 1.0 : (ax == 2 ? (double)S.q2[8] : (double)S.q2[9 + ax - 3]);
      const double be = ax < 2 ? dt2 * lam[ax] : dt2 * (double)S.q2[ax];  // q_theta_z / q_p: q2[2..5]
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        const int M = ri > k ? ri : k;
        const double T0 = (double)(N - M), ia = (double)(M - ri), ib = (double)(M - k);
        const double S1 = 0.5 * T0 * (T0 - 1.0), S2 = (T0 - 1.0) * T0 * (2.0 * T0 - 1.0) / 6.0;
        const double K2 = S2 + (ia + ib) * S1 + ia * ib * T0;
        row[k] = (live && k < N) ? fma(al, T0, be * K2) : (k == ri ? 1.0 : 0.0);
      }
    }
    // in-place Gauss-Jordan, the pivot row through LDS (double-buffered in the
    // table area, which is written only after the last pivot)
    double *xch = reinterpret_cast<double *>(&S.gtab[0][0][0]);
    static_assert(sizeof(S.gtab) >= 2 * 6 * NS * sizeof(double), "pivot-row exchange fits the table area");
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      if (k >= N) continue;  // uniform; not a break (the loop must unroll: row[] stays in registers)
      double *buf = xch + (k & 1) * (6 * NS);
      if (live && ri == k) {
#pragma unroll
        for (int c = 0; c < NS; ++c) buf[ax * NS + c] = row[c];
      }
      bsync<W>();
      const double *pr = buf + ax * NS;  // the pivot row, read as it is used (no second register row)
      const double pinv = 1.0 / pr[k];
      const double fk = row[k] * pinv;
#pragma unroll
      for (int c = 0; c < NS; ++c) {
        if (c == k) continue;
        const double pc = pr[c];
        row[c] = ri == k ? pc * pinv : fma(-fk, pc, row[c]);
      }
      row[k] = ri == k ? pinv : -fk;
    }
    bsync<W>();
    // the padding entries of the tables are zero
    for (int idx = tid; idx < NT * NT * 3; idx += 64 * W) (&S.gtab[0][0][0])[idx] = (f2v)(0.0f);
    bsync<W>();
    float dmax = 0.0f;
    if (live) {
      const int csi = W == 1 ? ri : (ri < H ? ri : 10 + ri - H);
      float *dst = reinterpret_cast<float *>(&S.gtab[csi][0][0]);
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        if (k < N) {
          const int csk = W == 1 ? k : (k < H ? k : 10 + k - H);
          dst[csk * 6 + ax] = (float)row[k];
        }
        // world-frame diagonal of the xy block <= 2 max_a |S[.][a]|^2 A_a^-1(j, j)
        dmax = k == ri ? (float)(sn2 * row[k]) : dmax;
      }
    }
    if (tid == 0) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) S.sc[wv].sxy[i][j] = (float)sxy[i][j];
    }
    if constexpr (W == 2) {
      if (tid == 64) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) S.sc[1].sxy[i][j] = (float)sxy[i][j];
      }
    }
    gmx = sgpr_f(bmax1<W>(S, wmax_nonneg(dmax), wv));
    bsync<W>();
  }
  for (;;) {
    // ---------------- 6a. factorisation for the current rho
    {
      // opaque per factorisation: nothing derived from these is hoisted out of
      // the refactor loop (it would stay live through the ADMM iterations)
      int ln = fresh_lane();
      asm volatile("" : "+v"(ln));
      const float rho = uf(S.sc[wv].rho), cinv = uf(S.sc[wv].cinv), sigma = uf(S.sc[wv].sigma);
      QL_LIT_LANE_INDICES(lxf);
      // this lane's row of W0^-1 for slot h (W0 = D^-1 (sigma I + A~' rho A~) D^-1 +
      // c R, 3 x 3 per leg): written to w0i for the U rows, and read back from
      // there for the iteration coefficients after the inversion
      auto w0_inv_row = [&](int h, float &i0, float &i1, float &i2) {
        const float dinv_h = valid[h] ? 1.0f / S.dr[wv][h][lxf] : 0.0f, csw = uf(S.sc[wv].cs);
        const f4v arz = S.arz[wv][h][lxf];
        const float rv0 = eq0[h] ? 1e3f * rho : rho, rv1 = rho;
        const float d_own = rv0 * arz.x * arz.x + rv1 * arz.y * arz.y;
        const float d_oz = rv0 * arz.x * arz.z + rv1 * arz.y * arz.w;
        const float d_zz = rv0 * arz.z * arz.z + rv1 * arz.w * arz.w;
        const float oz1 = lane_prev(d_oz), oz2 = lane_prev(oz1);
        const float zz1 = lane_prev(d_zz), zz2 = lane_prev(zz1);
        float m0, m1, m2;  // this lane's row of sigma I + A~' rho A~ (scaled space)
        if (comp == 0) {
          m0 = d_own + sigma; m1 = 0.0f; m2 = d_oz;
        } else if (comp == 1) {
          m0 = 0.0f; m1 = d_own + sigma; m2 = d_oz;
        } else {
          m0 = oz2; m1 = oz1; m2 = d_own + zz1 + zz2 + sigma;
        }
        const Triple dd = triple(dinv_h, comp);
        // W0 row = D^-1 M D^-1 + c R (diagonal)
        float w0 = dinv_h * m0 * dd.v0, w1 = dinv_h * m1 * dd.v1, w2 = dinv_h * m2 * dd.v2;
        const float cr = csw * (valid[h] ? S.r2[3 * leg[h] + comp] : 0.0f);
        w0 += comp == 0 ? cr : 0.0f;
        w1 += comp == 1 ? cr : 0.0f;
        w2 += comp == 2 ? cr : 0.0f;
        if (!valid[h]) { w0 = comp == 0 ? 1.0f : 0.0f; w1 = comp == 1 ? 1.0f : 0.0f; w2 = comp == 2 ? 1.0f : 0.0f; }
        // the full 3 x 3 leg block: rows from the triple's lanes
        const Triple c0 = triple(w0, comp), c1 = triple(w1, comp), c2 = triple(w2, comp);
        // rows: row0 = (c0.v0, c1.v0, c2.v0), row1 = (c0.v1, ...), row2 = (c0.v2, ...)
        const float a00 = c0.v0, a01 = c1.v0, a02 = c2.v0;
        const float a10 = c0.v1, a11 = c1.v1, a12 = c2.v1;
        const float a20 = c0.v2, a21 = c1.v2, a22 = c2.v2;
        const float k00 = a11 * a22 - a12 * a21, k01 = a02 * a21 - a01 * a22, k02 = a01 * a12 - a02 * a11;
        const float k10 = a12 * a20 - a10 * a22, k11 = a00 * a22 - a02 * a20, k12 = a02 * a10 - a00 * a12;
        const float k20 = a10 * a21 - a11 * a20, k21 = a01 * a20 - a00 * a21, k22 = a00 * a11 - a01 * a10;
        const float idet = 1.0f / (a00 * k00 + a01 * k10 + a02 * k20);
        i0 = (comp == 0 ? k00 : (comp == 1 ? k10 : k20)) * idet;  // row comp of W0^-1
        i1 = (comp == 0 ? k01 : (comp == 1 ? k11 : k21)) * idet;
        i2 = (comp == 0 ? k02 : (comp == 1 ? k12 : k22)) * idet;
      };
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float i0, i1, i2;
        w0_inv_row(h, i0, i1, i2);
        S.w0i[wv][0][h][lxf] = i0;
        S.w0i[wv][1][h][lxf] = i1;
        S.w0i[wv][2][h][lxf] = i2;
      }
      lsync();
      // U_j rows: wrench lane (jr, sr): U[sr][t] = sum_w Bb[sr][w] (W0^-1 Bb')[w][t]
      float Urow[6];  // this lane's row of U_jr, in registers (padding lanes: identity)
      {
        float yv[12];
        const int hh = jr >= 5 ? 1 : 0, base = 12 * (jr - 5 * hh);
#pragma unroll
        for (int g = 0; g < 4; ++g) {  // leg g of the step: 3 x 3 block
          const int v0 = base + 3 * g;
          const f4v r0 = {S.w0i[wv][0][hh][v0], S.w0i[wv][1][hh][v0], S.w0i[wv][2][hh][v0], 0.0f},
                    r1 = {S.w0i[wv][0][hh][v0 + 1], S.w0i[wv][1][hh][v0 + 1], S.w0i[wv][2][hh][v0 + 1], 0.0f},
                    r2 = {S.w0i[wv][0][hh][v0 + 2], S.w0i[wv][1][hh][v0 + 2], S.w0i[wv][2][hh][v0 + 2], 0.0f};
          const float b0 = S.Bb[sr][3 * g], b1 = S.Bb[sr][3 * g + 1], b2 = S.Bb[sr][3 * g + 2];
          yv[3 * g + 0] = b0 * r0.x + b1 * r1.x + b2 * r2.x;
          yv[3 * g + 1] = b0 * r0.y + b1 * r1.y + b2 * r2.y;
          yv[3 * g + 2] = b0 * r0.z + b1 * r1.z + b2 * r2.z;
        }
#pragma unroll
        for (int t = 0; t < 6; ++t) {
          float acc = 0.0f;
#pragma unroll
          for (int w = 0; w < 12; ++w) acc = fmaf(yv[w], S.Bb[t][w], acc);
          Urow[t] = wvalid ? acc : (t == sr ? 1.0f : 0.0f);
        }
      }
      // T = (I + cG U)^-1 cG = (U + (cG)^-1)^-1: this lane's
      // row of M = G^-1 / c + U (G^-1 from the per-solve tables through the
      // omega block's rotation; U block-diagonal: this lane's row of U_jr in
      // its own step's six columns), scaled by 1 / (max diag G^-1 / c + max
      // diag U) -- a bound within 2x of max diag M (SPD) -- and inverted in
      // place.  (Round 4's S = I + L'cGL form left a KKT backward error of
      // 1e-3 .. 1e-2 at rho <= 3e-4; M keeps it at 1e-5 .. 5e-4,
      // tools/lit_numerics.py.)
      float sM;
      {
        float uii = 0.0f;
#pragma unroll
        for (int t = 0; t < 6; ++t) uii = t == sr ? Urow[t] : uii;
        sM = sgpr_f(1.0f / fmaf(gmx, cinv, bmax1<W>(S, wmax_nonneg(wvalid ? uii : 0.0f), wv)));
        // omega x / y block coefficients S[sr][a] S[t][a], a, t in {0, 1}
        // (the G^-1 tables hold the eigen axes' A_a^-1)
        const float s00 = uf(S.sc[wv].sxy[0][0]), s01 = uf(S.sc[wv].sxy[0][1]), s10 = uf(S.sc[wv].sxy[1][0]),
                    s11 = uf(S.sc[wv].sxy[1][1]);
        // padding wrench lanes (identity rows: unit entry, unit U) carry zero
        // coefficients, so their G^-1 terms are exact zeros, and the unit entry
        // joins the own-block addend below: one select per entry
        const float r0 = !wvalid ? 0.0f : (sr == 0 ? s00 : (sr == 1 ? s10 : 0.0f)),
                    r1 = !wvalid ? 0.0f : (sr == 0 ? s01 : (sr == 1 ? s11 : 0.0f));
        const float c00 = r0 * s00, c01 = r0 * s10, c10 = r1 * s01, c11 = r1 * s11;
        const float m2 = (wvalid && sr == 2) ? 1.0f : 0.0f, m3 = (wvalid && sr == 3) ? 1.0f : 0.0f,
                    m4 = (wvalid && sr == 4) ? 1.0f : 0.0f, m5 = (wvalid && sr == 5) ? 1.0f : 0.0f;
        const float scale = sM * cinv;
        // the own step block's addend per column: sM U (a valid row; fma(scale,
        // 0, v) is v), or the padding row's whole entry fma(scale, 1, sM) on its
        // diagonal (lanes 60 .. 63 hold no row: no unit entry)
        const float unit = (!wvalid && ln < 60) ? 1.0f : 0.0f;
        float own_add[6];
#pragma unroll
        for (int t = 0; t < 6; ++t) own_add[t] = fmaf(scale, t == sr ? unit : 0.0f, sM * Urow[t]);
#pragma unroll
        for (int wp = 0; wp < W; ++wp) {
#pragma unroll
          for (int k = 0; k < kLitN; ++k) {
            const f2v e0 = S.gtab[jc][10 * wp + k][0], e1 = S.gtab[jc][10 * wp + k][1],
                      e2 = S.gtab[jc][10 * wp + k][2];
            const float gv[6] = {fmaf(c00, e0.x, c10 * e0.y), fmaf(c01, e0.x, c11 * e0.y), m2 * e1.x,
                                 m3 * e1.y, m4 * e2.x, m5 * e2.y};
            const bool blk = wp == wv && k == jr;  // this row's own step block
#pragma unroll
            for (int t = 0; t < 6; ++t) {
              const int c = 60 * wp + 6 * k + t;
              T.k[c] = fmaf(scale, gv[t], blk ? own_add[t] : 0.0f);
              asm volatile("" : "+v"(T.k[c]));  // final here (no sinking into the Gauss-Jordan)
            }
          }
        }
#pragma unroll
        for (int c = 60 * W; c < 64 * W; ++c) T.k[c] = 0.0f;
      }
      if constexpr (W == 1)
        lit_invert(nw, T);  // (sM M)^-1
      else
        lit_invert2(S, wv, 6 * H, 6 * (N - H), T);
#pragma unroll
      for (int c = 0; c < 60 * W; ++c) T.k[c] *= sM;  // T = M^-1
      // a = W0^-1 D^-1 b and x~ = D^-1 (a - W0^-1 t): this lane's row of W0^-1
      // as leg-triple shifts (D^-1 applied elementwise around the two dots)
#pragma unroll
      // (the rows written for U above, read back: the inversion works in
      // registers (two waves: and S.bc), so w0i still holds them)
      for (int h = 0; h < 2; ++h) {
        const float wx = S.w0i[wv][0][h][lxf], wy = S.w0i[wv][1][h][lxf], wz = S.w0i[wv][2][h][lxf];
        W1[h] = shift5(valid[h] ? wx : 0.0f, valid[h] ? wy : 0.0f, valid[h] ? wz : 0.0f, comp);
      }
    }
    bool refactor = false;

    for (;;) {
      int iter = ui(S.sc[wv].iter);
      const int ctm = ui(S.sc[wv].ctm), interval = ui(S.sc[wv].interval);
      if (iter < a.max_iter) {
        int next = a.max_iter;
        if (ctm) next = min(next, (iter / ctm + 1) * ctm);
        if (interval) next = min(next, (iter / interval + 1) * interval);
        const float rho = uf(S.sc[wv].rho);
        const float rho_s = rho;
        const float rvb_s = sgpr_f(1.0f / rho);
        const float zlo = uf(S.sc[wv].zlo);  // z rows: lower = zlo upper (from LDS: no register across the phases)
        QL_LIT_LANE_INDICES(lxi);
        // loop operands read here, per segment of iterations: none is a register
        // across the residual checks and factorisations
        const float alpha = uf(S.sc[wv].alpha), oma = uf(S.sc[wv].oma), sigma = uf(S.sc[wv].sigma),
                    dtm = uf(S.sc[wv].dtm);
        // (q~ and D^-1 are carried like (ra, rz) below: read again every
        // iteration, registers only from there to the next av write, free while
        // v = Vu a holds its operands.  D^-1 is parked in w0i, which is the
        // factorisation's and idle between two of them.)
        float qvr[2], Dinv[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          qvr[h] = S.qvl[wv][h][lxi];
          Dinv[h] = valid[h] ? 1.0f / S.dr[wv][h][lxi] : 0.0f;
          S.w0i[wv][0][h][lxi] = Dinv[h];
          // the first row's lower bound (0 on x / y rows, zlo zh on z rows) is
          // constant for the solve: parked beside D^-1 and read next to zh, so
          // neither a multiply and a select per iteration nor a loop register
          S.w0i[wv][1][h][lxi] = xy ? 0.0f : zlo * S.zh[wv][h][lxi];
        }
        // rho vector (eq rows 1e3 rho) of the slots' first rows and its inverse,
        // held for the segment (four registers; the second rows' rho is the scalar)
        float rva0[2], rvia[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          rva0[h] = eq0[h] ? 1e3f * rho_s : rho_s;
          rvia[h] = eq0[h] ? 1e-3f * rvb_s : rvb_s;
          asm volatile("" : "+v"(rva0[h]), "+v"(rvia[h]));
        }
        // wave-uniform trip count (a scalar loop, not an exec-masked one)
        iter = __builtin_amdgcn_readfirstlane(iter);
        next = __builtin_amdgcn_readfirstlane(next);
        // One iteration has three LDS round trips that the algorithm needs
        // (av, the broadcast row, wv: each written and read back); every other
        // LDS read is of data constant since the set-up and is issued where
        // arithmetic or the matvec hides its latency:
        //  - a slot's (ra, rz) is read once per iteration, under the second
        //    W0^-1 product, used by update_z and carried over the back-edge
        //    into the next iteration's rhs (read here for the segment's first);
        //  - this lane's row of Bb is read ahead of the av write; the
        //    variables' Bb columns, a and D^-1 under the matvec; zh and q~
        //    under the W0^-1 products of update_x;
        //  - the two slots' chains run stage by stage, side by side: a DPP
        //    operand is then two instructions behind its producer.
        __builtin_amdgcn_sched_barrier(0);  // (after the segment's index arithmetic, not among it)
        f4v arzc[2] = {S.arz[wv][0][lxi], S.arz[wv][1][lxi]};
        const uint64_t xym = __builtin_amdgcn_ballot_w64(xy);
        for (; iter < next; ++iter) {
          asm volatile("" ::: "memory");
          const int par = W == 1 ? 0 : (iter & 1);  // two waves: broadcast rows double-buffered
          const float rva[2][2] = {{rva0[0], rho_s}, {rva0[1], rho_s}};
          const float rvb = rvb_s;
          // rhs = sigma x - q + A'(rho z - y) per slot, then a = W0^-1 D^-1 rhs
          float av[2];
          float tz[2], rhs[2];
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const f2v ra = {arzc[h].x, arzc[h].y}, rz = {arzc[h].z, arzc[h].w};
            const f2v rv = {rva[h][0], rva[h][1]};
            const f2v w = __builtin_elementwise_fma(rv, z[h], -y[h]);
            const f2v aw = ra * w, zw = rz * w;
            tz[h] = zw.x + zw.y;
            rhs[h] = fmaf(sigma, x[h], (aw.x + aw.y) - qvr[h]);
          }
          // this wrench lane's row of Bb for v = Vu a below
          const f4v *br = reinterpret_cast<const f4v *>(S.Bb[sr]);
          const f4v b0 = br[0], b1 = br[1], b2 = br[2];
          __builtin_amdgcn_sched_barrier(0);
          {
            // both slots: rhs += [comp == 2] (tz(l - 1) + tz(l - 2)), t = D^-1 rhs,
            // a = W0^-1 t (tdot's five terms in tdot's order)
            // (the z rows' mask as a float: made here, not a register of the loop)
            float m2, u0, u1, t0, t1;
            asm volatile("v_cndmask_b32_e64 %0, 1.0, 0, %1" : "=v"(m2) : "s"(xym));
            asm("s_nop 1\n\t"
                "v_add_f32_dpp %2, %8, %8 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
                "v_add_f32_dpp %3, %9, %9 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
                "s_nop 0\n\t"
                "v_fmac_f32_dpp %4, %2, %10 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
                "v_fmac_f32_dpp %5, %3, %10 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
                "v_mul_f32 %6, %11, %4\n\t"
                "v_mul_f32 %7, %12, %5\n\t"
                "s_nop 0\n\t"
                "v_mov_b32_dpp %2, %6 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
                "v_mov_b32_dpp %3, %7 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
                "v_mov_b32_dpp %4, %6 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
                "v_mov_b32_dpp %5, %7 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
                "v_mul_f32 %0, %6, %13\n\t"
                "v_mul_f32 %1, %7, %18\n\t"
                "v_fmac_f32_dpp %0, %6, %14 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
                "v_fmac_f32_dpp %1, %7, %19 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
                "v_fmac_f32_dpp %0, %6, %16 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
                "v_fmac_f32_dpp %1, %7, %21 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
                "v_fmac_f32_dpp %0, %2, %15 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
                "v_fmac_f32_dpp %1, %3, %20 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
                "v_fmac_f32_dpp %0, %4, %17 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
                "v_fmac_f32_dpp %1, %5, %22 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:0"
                : "=&v"(av[0]), "=&v"(av[1]), "=&v"(u0), "=&v"(u1), "+v"(rhs[0]), "+v"(rhs[1]), "=&v"(t0), "=&v"(t1)
                : "v"(tz[0]), "v"(tz[1]), "v"(m2), "v"(Dinv[0]), "v"(Dinv[1]),
                  "v"(W1[0].c0), "v"(W1[0].cm1), "v"(W1[0].cm2), "v"(W1[0].cp1), "v"(W1[0].cp2),
                  "v"(W1[1].c0), "v"(W1[1].cm1), "v"(W1[1].cm2), "v"(W1[1].cp1), "v"(W1[1].cp2));
          }
          S.av[wv][0][lxi] = av[0];
          S.av[wv][1][lxi] = av[1];
          lsync();
          // v = Vu a: wrench row (jr, sr) over its step's 12 variables
          float wr = 0.0f;
          {
            const int hh = jr >= 5 ? 1 : 0, base = 12 * (jr - 5 * hh);
            const f4v *src = reinterpret_cast<const f4v *>(&S.av[wv][hh][base]);
            // (one wave at 128 registers: the third quarter is read into the
            // registers the first one leaves -- 20 operands live, not 24)
            const f4v u0 = src[0], u1 = src[1];
            f4v u2;
            if constexpr (W == 2) u2 = src[2];
            __builtin_amdgcn_sched_barrier(0);
            float w0 = 0.0f, w1 = 0.0f;
            w0 = fmaf(b0.x, u0.x, w0);
            w1 = fmaf(b0.y, u0.y, w1);
            w0 = fmaf(b0.z, u0.z, w0);
            w1 = fmaf(b0.w, u0.w, w1);
            if constexpr (W == 1) {
              __builtin_amdgcn_sched_barrier(0);
              u2 = src[2];
              __builtin_amdgcn_sched_barrier(0);
            }
            w0 = fmaf(b1.x, u1.x, w0);
            w1 = fmaf(b1.y, u1.y, w1);
            w0 = fmaf(b1.z, u1.z, w0);
            w1 = fmaf(b1.w, u1.w, w1);
            w0 = fmaf(b2.x, u2.x, w0);
            w1 = fmaf(b2.y, u2.y, w1);
            w0 = fmaf(b2.z, u2.z, w0);
            w1 = fmaf(b2.w, u2.w, w1);
            wr = w0 + w1;
          }
          reinterpret_cast<float *>(&S.bc[par][wv][0])[lxi] = wr;
          bsync<W>();
          // s = T v (DPP broadcast matvec, 60 columns per half); under it the
          // reads update_x / update_z need that do not depend on s: the
          // variable's omega rows of B_d (a padding slot's are harmless: its
          // leg's W0^-1 coefficients are zero), a and D^-1
          float sv;
          float bw0, bw1, bw2, zhi[2], zlw[2], avr[2];
          {
            const f4v r0 = S.bc[par][0][lxi & 15];
            f4v r1;
            if constexpr (W == 2) r1 = S.bc[par][1][lxi & 15];
            bw0 = S.Bb[0][lxi % 12], bw1 = S.Bb[1][lxi % 12], bw2 = S.Bb[2][lxi % 12];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              avr[h] = S.av[wv][h][lxi];  // a, as written above: read back, not held across v = Vu a
              Dinv[h] = S.w0i[wv][0][h][lxi];
            }
            __builtin_amdgcn_sched_barrier(0);
            float acc0, acc1;
            QL_DPP_MATVEC60_2(acc0, acc1, r0, T.k, 0);
            if constexpr (W == 2) {
              float acc2, acc3;
              QL_DPP_MATVEC60_2(acc2, acc3, r1, T.k, 60);
              sv = (acc0 + acc1) + (acc2 + acc3);
            } else {
              sv = acc0 + acc1;
            }
          }
          S.wv[wv][lxi] = sv;
          lsync();
          // x~ = D^-1 a - D^-1 W0^-1 Vu' s, then update_x / update_z / update_y:
          // both slots' wrench triples under one wait, the chains side by side
          // (the step's omega rows and the variable's own v row, the latter by
          // its lane address: no select.  Slot 1's step is slot 0's + 5, so one
          // pair of address registers serves both slots; a padding slot 1 reads
          // finite values that its zero W0^-1 coefficients drop.)
          f2v s01[2];
          float s2[2], sf[2];
          {
            const float *gs = &S.wv[wv][6 * stepl[0]], *gc = gs + 3 + comp;
#pragma unroll
            for (int h = 0; h < 2; ++h) sf[h] = gc[30 * h];  // issued in the order the sums below take them
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int h = 0; h < 2; ++h) s2[h] = gs[30 * h + 2];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int h = 0; h < 2; ++h) s01[h] = *reinterpret_cast<const f2v *>(gs + 30 * h);
            __builtin_amdgcn_sched_barrier(0);
          }
          float tv[2], td[2];
#pragma unroll
          for (int h = 0; h < 2; ++h)
            tv[h] = fmaf(bw0, s01[h].x, fmaf(bw1, s01[h].y, fmaf(bw2, s2[h], dtm * sf[h])));
          // (ra, rz) for update_z and the next iteration's rhs: into the registers
          // the wrench triples leave, under the two W0^-1 products
          asm volatile("" : "+v"(tv[0]), "+v"(tv[1]));
          arzc[0] = S.arz[wv][0][lxi];
          arzc[1] = S.arz[wv][1][lxi];
          __builtin_amdgcn_sched_barrier(0);
          tdot2(tv[0], W1[0], tv[1], W1[1], td[0], td[1]);
          // the upper bounds, and q~ for the next iteration's rhs
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            zhi[h] = S.zh[wv][h][lxi];
            zlw[h] = S.w0i[wv][1][h][lxi];
            qvr[h] = S.qvl[wv][h][lxi];
          }
          // (stage by stage over the two slots, like the chains above: a packed
          // result is not the next instruction's operand)
          float xt[2], xtz[2];
          f2v zt[2], zr[2], vv[2], zn[2];
#pragma unroll
          for (int h = 0; h < 2; ++h) xt[h] = Dinv[h] * (avr[h] - td[h]);  // D^-1 (a - W0^-1 t)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const float n1 = lane_next(xt[h]), n2 = lane_next(n1);
            xtz[h] = comp == 0 ? n2 : n1;
            x[h] = fmaf(alpha, xt[h], oma * x[h]);
          }
          asm volatile("" : "+v"(arzc[0]), "+v"(arzc[1]));  // both quads under one wait
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const f2v ra = {arzc[h].x, arzc[h].y}, rz = {arzc[h].z, arzc[h].w};
            zt[h] = __builtin_elementwise_fma(rz, (f2v)(xtz[h]), ra * xt[h]);
          }
#pragma unroll
          for (int h = 0; h < 2; ++h) zr[h] = __builtin_elementwise_fma((f2v)(alpha), zt[h], oma * z[h]);
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const f2v rvi2 = {rvia[h], rvb};
            vv[h] = __builtin_elementwise_fma(y[h], rvi2, zr[h]);
          }
#pragma unroll
          for (int h = 0; h < 2; ++h)
            zn[h] = {__builtin_amdgcn_fmed3f(vv[h].x, zlw[h], zhi[h]), __builtin_amdgcn_fmed3f(vv[h].y, -INFINITY, 0.0f)};
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const f2v rv = {rva[h][0], rva[h][1]};
            y[h] = __builtin_elementwise_fma(rv, zr[h] - zn[h], y[h]);
            z[h] = zn[h];
          }
        }
      }
      iter = ui(iter);
      S.sc[wv].iter = iter;
      const bool fin = iter >= a.max_iter;
      const bool can_check = ctm && iter > 0 && (iter % ctm == 0);
      const bool do_rho = interval && iter > 0 && (iter % interval == 0);
      if (!(can_check || do_rho || fin)) continue;
      float o[6], r[6];
      residuals(o, r, do_rho);
      const float cinv = uf(S.sc[wv].cinv), qn0 = uf(S.sc[wv].qn0);
      const float pri_res = o[0], dua_res = cinv * o[3];
      if (can_check) {
        const float eps_p = a.eps_abs + a.eps_rel * fmaxf(o[1], o[2]);
        const float eps_d = a.eps_abs + a.eps_rel * cinv * fmaxf(fmaxf(qn0, o[4]), o[5]);
        if (pri_res < eps_p && dua_res < eps_d) {
          S.sc[wv].status = QLOCO_OK;
          break;
        }
      }
      if (do_rho) {  // compute_rho_estimate + adapt_rho
        const float pn = r[0] / (fmaxf(r[1], r[2]) + 1e-30f);
        const float dn = r[3] / (fmaxf(fmaxf(uf(S.sc[wv].qn1), r[4]), r[5]) + 1e-30f);
        const float rho = uf(S.sc[wv].rho);
        float rho_new = rho * sqrtf(pn / (dn + 1e-30f));
        rho_new = fminf(fmaxf(rho_new, 1e-6f), 1e6f);
        if (rho_new > rho * a.rho_tol || rho_new < rho / a.rho_tol) {
          const int nup = ui(S.sc[wv].rho_updates) + 1;
          S.sc[wv].rho = sgpr_f(rho_new);
          S.sc[wv].rho_updates = nup;
          if (!fin) {
            refactor = true;
            break;
          }
        }
      }
      if (fin) {
        float e_abs = a.eps_abs, e_rel = a.eps_rel;  // laundered: 10 eps is not hoisted into VGPRs
        asm volatile("" : "+v"(e_abs), "+v"(e_rel));
        const float ep = 10.f * e_abs + 10.f * e_rel * fmaxf(o[1], o[2]);
        const float ed = 10.f * e_abs + 10.f * e_rel * cinv * fmaxf(fmaxf(qn0, o[4]), o[5]);
        S.sc[wv].status = __builtin_amdgcn_readfirstlane((pri_res < ep && dua_res < ed) ? QLOCO_SOLVED_INACCURATE
                                                                                          : QLOCO_MAX_ITER);
        break;
      }
    }
    if (!refactor) break;
  }

  // ---------------- 7. outputs: unscale, objective, leg slots (A1RobotControl.cpp:593-599)
  const int lane_o = fresh_lane();
  const int tid_o = W == 1 ? lane_o : (int)threadIdx.x;
  float xu[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) xu[h] = valid[h] ? x[h] * S.dr[wv][h][lane_o] : 0.0f;
  // P~ x at the final iterate, recomputed (the last check's copy would be a
  // register live across every ADMM iteration; same operands, same result)
  float px[2];
  p_times_x(px);
  const float cinv = uf(S.sc[wv].cinv);
  int status = ui(S.sc[wv].status);
  float ob = 0.0f;
#pragma unroll
  for (int h = 0; h < 2; ++h) ob += valid[h] ? cinv * (0.5f * x[h] * px[h] + S.qvl[wv][h][lane_o] * x[h]) : 0.0f;
  const float objp = bsum<W>(S, wsum(ob), wv);
  const bool bad = !isfinite(objp);
  if (bad) status = QLOCO_NAN;
  if (a.u) {
    float *uo = a.u + b * 12 * N + 12 * so;
#pragma unroll
    for (int h = 0; h < 2; ++h)
      if (valid[h]) uo[60 * h + lane_o] = bad ? NAN : xu[h];
  }
  // u0: step-0 forces (variables 0..11 = wave 0's slot 0, lanes 0..11); optional body frame R' u
  {
    const float n1 = lane_next(xu[0]), n2 = lane_next(n1);
    const float p1 = lane_prev(xu[0]), p2 = lane_prev(p1);
    const float f0 = comp == 0 ? xu[0] : (comp == 1 ? p1 : p2);
    const float f1 = comp == 0 ? n1 : (comp == 1 ? xu[0] : p1);
    const float f2 = comp == 0 ? n2 : (comp == 1 ? n1 : xu[0]);
    if (tid_o < 12) {
      float o = xu[0];
      if (a.output_frame == 1) {  // R^T f with R = [[c,s,0],[-s,c,0],[0,0,1]], recomputed here
        const float yw = S.x0[2], cw = cosf(yw), sw = sinf(yw);
        o = comp == 0 ? (cw * f0 - sw * f1) : (comp == 1 ? (sw * f0 + cw * f1) : f2);
      }
      a.u0[b * 12 + lane_o] = bad ? NAN : o;
    }
  }
  if (prec) {  // the persistent record for the next call (layout QLOCO_SRBD_PERSIST_LEN)
    QL_LIT_LANE_INDICES(lxo);  // fresh indices: no address kept live from the warm start
    for (int k = tid_o; k < NP + 4; k += 64 * W)
      if (k < 84 * N || k >= 96 * N) prec[k] = 0.0f;  // [84 N, 96 N): q, written at the gradient
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (!valid[h]) continue;
      const int vidx = 12 * step[h] + 3 * leg[h] + comp, rbase = 20 * step[h] + 5 * leg[h] + 2 * comp;
      prec[vidx] = x[h];
      prec[52 * N + vidx] = xu[h];
      prec[12 * N + rbase] = z[h].x;
      prec[32 * N + rbase] = y[h].x;
      const f2v e = row_e(h);
      prec[64 * N + rbase] = cinv * e.x * y[h].x;
      if (xy) {
        prec[12 * N + rbase + 1] = z[h].y;
        prec[32 * N + rbase + 1] = y[h].y;
        prec[64 * N + rbase + 1] = cinv * e.y * y[h].y;
      }
    }
    for (int k = tid_o; k < 4 * N; k += 64 * W) prec[96 * N + k] = S.ctf[k];
    if (tid_o == 0) {
      prec[NP] = S.sc[wv].rho;
      prec[NP + 1] = 1.0f;
    }
  }
  if (WS && a.warm_start == 1) {
    QL_LIT_LANE_INDICES(lxo);
    const int nu = 12 * N, ncn = 20 * N;
    float *wx = a.warm + b * (nu + ncn);
    float *wy = wx + nu;
    for (int k = tid_o; k < nu + ncn; k += 64 * W) wx[k] = 0.0f;
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (!valid[h]) continue;
      wx[12 * step[h] + 3 * leg[h] + comp] = xu[h];
      const int rbase = 20 * step[h] + 5 * leg[h] + 2 * comp;
      const f2v e = row_e(h);
      wy[rbase] = cinv * e.x * y[h].x;
      if (xy) wy[rbase + 1] = cinv * e.y * y[h].y;
    }
  }
  if (tid_o == 0) {
    if (a.status) a.status[b] = status;
    if (a.iters) a.iters[b] = S.sc[wv].iter;
    if (a.hint) a.hint[b] = S.sc[wv].iter;  // placement state: the next call's order
    if (a.rho_updates) a.rho_updates[b] = S.sc[wv].rho_updates;
    if (a.obj) a.obj[b] = objp;
  }
}

// One instance per workgroup.  srbd_lit_kernel / srbd_lit2_kernel are the
// kernels of a call without model rows (MR = false in srbd_lit_one),
// srbd_lit_rows_kernel / srbd_lit2_rows_kernel those of a call with rows; a
// pair shares its body as text, so the first two stay the kernels they were.
//
// One wave: the placement state's order (qloco_srbd_place.hpp) once it is
// ready for this batch: which workgroup solves an instance, never what it
// computes or where its outputs go.  The workgroup's rank is place_assign's
// (DESIGN.md §3r): uniform scalar arithmetic and two uniform loads
#define QL_LIT_KERNEL_BODY(MR)                                                                             \
  __shared__ __attribute__((aligned(16))) LitLds<1> S;                                                     \
  int64_t i = blockIdx.x;                                                                                  \
  if (a.order && a.hint[-kPlaceHeader] == a.batch) {                                                       \
    const int64_t at = place_position(place_assign(i, a.batch, a.place_simds), a.batch, a.place_simds);    \
    if (at < 0 || at >= a.batch) return;                                                                   \
    i = a.order[at];                                                                                       \
  }                                                                                                        \
  if (i < 0 || i >= a.batch) return;                                                                       \
  srbd_lit_one<1, WS, MR>(a, S, i)
#define QL_LIT2_KERNEL_BODY(MR)                           \
  __shared__ __attribute__((aligned(16))) LitLds<2> S;    \
  const int64_t i = blockIdx.x;                           \
  if (i >= a.batch) return;                               \
  srbd_lit_one<2, WS, MR>(a, S, i)

template <bool WS>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kLitWpe)))
void srbd_lit_kernel(const SrbdArgs a) {
  QL_LIT_KERNEL_BODY(false);
}

template <bool WS>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kLitWpe)))
void srbd_lit_rows_kernel(const SrbdArgs a) {
  QL_LIT_KERNEL_BODY(true);
}

template <bool WS>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(kLit2Wpe)))
void srbd_lit2_kernel(const SrbdArgs a) {
  QL_LIT2_KERNEL_BODY(false);
}

template <bool WS>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(kLit2Wpe)))
void srbd_lit2_rows_kernel(const SrbdArgs a) {
  QL_LIT2_KERNEL_BODY(true);
}

// SIMDs of the current device (four per compute unit), asked once per device
static int device_simds(int *simds) {
  constexpr int kDevs = 64;
  static int cached[kDevs];
  int dev = 0, cus = 0;
  QLOCO_HIP_CHECK(hipGetDevice(&dev), "hipGetDevice");
  if (dev >= 0 && dev < kDevs && cached[dev] > 0) {
    *simds = cached[dev];
    return QLOCO_OK;
  }
  QLOCO_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev),
                  "hipDeviceGetAttribute");
  *simds = 4 * cus;
  if (dev >= 0 && dev < kDevs) cached[dev] = *simds;
  return QLOCO_OK;
}

int srbd_lit_launch(const SrbdArgs &a, bool warm, int32_t *place, int simds, hipStream_t stream) {
  const dim3 grid((unsigned)a.batch);
  const bool rows = a.model != nullptr;
  if (a.N < 1 || a.N > kLitN2) return QLOCO_BAD_SIZE;
  if (a.N <= kLitN) {
    if (warm) {
      hipLaunchKernelGGL((rows ? srbd_lit_rows_kernel<true> : srbd_lit_kernel<true>), grid, dim3(64), 0,
                         stream, a);
    } else {
      // cold solves of a batch that is resident at once but fills more than
      // one wave slot per SIMD: the launch ends with its most loaded SIMD, so
      // the instances are placed by their last iteration counts
      SrbdArgs ap = a;
      bool placed = false;
      if (place) {
        if (simds <= 0) {
          const int rc = device_simds(&simds);
          if (rc != QLOCO_OK) return rc;
        }
        placed = a.batch > simds && a.batch <= (int64_t)kLitWpe * simds;
      }
      if (placed) {
        ap.hint = place + kPlaceHeader;
        ap.order = place + kPlaceHeader + a.batch;
        ap.place_simds = simds;
      }
      hipLaunchKernelGGL((rows ? srbd_lit_rows_kernel<false> : srbd_lit_kernel<false>), grid, dim3(64), 0,
                         stream, ap);
      QLOCO_HIP_CHECK(hipGetLastError(), "srbd_lit_kernel launch");
      if (placed) return srbd_place_launch(place, a.batch, simds, a.check_termination, stream);
    }
    QLOCO_HIP_CHECK(hipGetLastError(), "srbd_lit_kernel launch");
  } else {
    if (warm)
      hipLaunchKernelGGL((rows ? srbd_lit2_rows_kernel<true> : srbd_lit2_kernel<true>), grid, dim3(128), 0,
                         stream, a);
    else
      hipLaunchKernelGGL((rows ? srbd_lit2_rows_kernel<false> : srbd_lit2_kernel<false>), grid, dim3(128), 0,
                         stream, a);
    QLOCO_HIP_CHECK(hipGetLastError(), "srbd_lit2_kernel launch");
  }
  return QLOCO_OK;
}

}  // namespace qloco

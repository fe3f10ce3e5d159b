// qloco_nlp_core.hpp -- what the slow planner's translation units share
// (qloco_nlp.hip, qloco_nlp_tick.hip, qloco_nlp_node.hip; sections 14, 15 and
// 16 of include/qloco.h): the three resident records' layouts, the numerics
// CoM_height_solve's parity rests on, the dense-record copy and the parameter
// checks.  Every offset and every function below has this one definition.
// Compile with -ffp-contract=off: the operation order is the restatements'
// (tests/nlp_tick_ref.py, tests/nlp_node_ref.py), and the explicit fma calls
// of nlp_powers are part of the result.
//
// Prefixes: ST_ the step-timing record (section 14), TK_ the tick record
// (section 15), ND_ the node record and NS_ the node scratch (section 16).
#pragma once
#include <cmath>

#include "qloco_common.hpp"

namespace qloco {

// ---- layouts -------------------------------------------------------------
constexpr int NLP_NS = QLOCO_NLP_STEPS;
constexpr int64_t kNlpMaxBatch = (int64_t)1 << 24;

// section 14: ts[B*27] | tx[B*27], a row per robot (the layout
// qloco_support_phase takes), then ST_FIELDS field-major values per robot
// (field f of robot b at 54 B + f B + b)
constexpr int ST_REC = QLOCO_NLP_STATE;
enum { ST_TD = 0, ST_LXX = 27, ST_LYY = 54, ST_FX = 81, ST_FY = 108, ST_CXI = 135, ST_CVXI = 162, ST_CYI = 189,
       ST_CVYI = 216, ST_VARI = 243, ST_FEED = 247, ST_END = 253, ST_FIELDS = 255 };
static_assert(2 * NLP_NS + ST_FIELDS == ST_REC, "record length");

// section 15: field-major (field f of robot b at f B + b); a ring entry is
// (Rfoot xyz, Lfoot xyz).  After the records, the scratch the step-timing
// kernel writes when the caller passes no buffer: com[B*18], sched[B*4]
// (int32), status[B] (int32).
constexpr int TK_RING = QLOCO_NLP_TICK_RING;
constexpr int TK_REC = QLOCO_NLP_TICK_STATE;
enum { TK_BJX1 = 0, TK_RY = 1, TK_TEND = 2, TK_SW0 = 3, TK_LAST = 4, TK_FZ = 5, TK_LIFT = 32, TK_TX0 = 59,
       TK_RINGF = 86 };
static_assert(TK_RINGF + TK_RING * 6 == TK_REC, "record length");
enum { TK_S_COM = TK_REC, TK_S_SCHED = TK_REC + 18, TK_S_STATUS = TK_REC + 20, TK_WS = TK_REC + 21 };

// section 16: field-major; a ring entry is (tag, _zmpx_real, _zmpy_real).
// After the records, NS_ doubles per robot of scratch.
constexpr int ND_RING = QLOCO_NLP_NODE_RING;
constexpr int ND_REC = QLOCO_NLP_NODE_STATE;
constexpr int ND_SCR = QLOCO_NLP_NODE_SCRATCH;
constexpr int ND_ROWLEN = QLOCO_GAIT_MSG_LEN;
enum { ND_COUNT = 0, ND_LATCH = 1, ND_RESTART = 2, ND_STOP = 3, ND_COL = 4, ND_COR = 7, ND_RINGF = 10, ND_ROW = 154 };
static_assert(ND_RINGF + ND_RING * 3 == ND_ROW && ND_ROW + ND_ROWLEN == ND_REC, "record length");
enum { NS_CT = 0, NS_RL = 38, NS_COM = 56, NS_VARI = 74, NS_EST = 78, NS_RF = 84, NS_LF = 86, NS_PREV = 88, NS_INT = 90 };
static_assert(NS_INT + 4 == ND_SCR, "scratch length");

// ---- numerics ------------------------------------------------------------
// (int)v of the reference, -1 where the conversion is undefined
__device__ __forceinline__ int nlp_int(double v) { return (v > -1.0e9 && v < 1.0e9) ? (int)v : -1; }

// the same with 0 out of range: the SQP's _tx index (:714-716), which is
// subtracted from the tick and never used as an array index
__device__ __forceinline__ int nlp_int_or_zero(double v) { return (v > -1.0e9 && v < 1.0e9) ? (int)v : 0; }

// entry k of a 27-vector, NaN outside it
__device__ __forceinline__ double nlp_at(const double *p, int64_t stride, int k) {
  return (k >= 0 && k < NLP_NS) ? p[(int64_t)k * stride] : __builtin_nan("");
}

// t^2 .. t^6 as pow() returns them: each power is carried as an unevaluated
// sum of two doubles (exact products through fma), so its leading part is the
// correctly rounded value
__device__ __forceinline__ void nlp_powers(double t, double (&p)[7]) {
  p[0] = 1.0;
  p[1] = t;
  double h = t * t, l = __builtin_fma(t, t, -h);
  p[2] = h;
#pragma unroll
  for (int n = 3; n <= 6; ++n) {
    const double q = h * t;
    const double e = __builtin_fma(h, t, -q) + l * t;
    h = q + e;
    l = e - (h - q);
    p[n] = h;
  }
}

// partial-pivot LU of a (in place) with the rows of r carried along: the pivot
// search and the swaps are selects over compile-time indices, so the matrix
// stays in registers.  Also the host's, for the squat polynomial.
template <int N, int M>
__host__ __device__ __forceinline__ void nlp_lu(double (&a)[N][N], double (&r)[N][M]) {
#pragma unroll
  for (int k = 0; k < N; ++k) {
    int p = k;
    double best = fabs(a[k][k]);
#pragma unroll
    for (int q = k + 1; q < N; ++q) {
      const double v = fabs(a[q][k]);
      const bool g = v > best;
      p = g ? q : p;
      best = g ? v : best;
    }
#pragma unroll
    for (int q = k + 1; q < N; ++q) {
      const bool s = p == q;
#pragma unroll
      for (int c = 0; c < N; ++c) {
        const double x = a[k][c], y = a[q][c];
        a[k][c] = s ? y : x;
        a[q][c] = s ? x : y;
      }
#pragma unroll
      for (int c = 0; c < M; ++c) {
        const double x = r[k][c], y = r[q][c];
        r[k][c] = s ? y : x;
        r[q][c] = s ? x : y;
      }
    }
#pragma unroll
    for (int q = k + 1; q < N; ++q) {
      a[q][k] = a[q][k] / a[k][k];
#pragma unroll
      for (int c = k + 1; c < N; ++c) a[q][c] = a[q][c] - a[q][k] * a[k][c];
    }
  }
}

// forward and back substitution of every column of r
template <int N, int M>
__host__ __device__ __forceinline__ void nlp_lu_solve(const double (&a)[N][N], double (&r)[N][M]) {
#pragma unroll
  for (int m = 0; m < M; ++m) {
#pragma unroll
    for (int q = 0; q < N; ++q) {
      double acc = r[q][m];
#pragma unroll
      for (int c = 0; c < q; ++c) acc = acc - a[q][c] * r[c][m];
      r[q][m] = acc;
    }
#pragma unroll
    for (int q = N - 1; q >= 0; --q) {
      double acc = r[q][m];
#pragma unroll
      for (int c = q + 1; c < N; ++c) acc = acc - a[q][c] * r[c][m];
      r[q][m] = acc / a[q][q];
    }
  }
}

// AAA (:2386-2412, :3599-3625): row q is the position (kind 0), velocity (1)
// or acceleration (2) row of the sextic at plan time `which`; its right-hand
// sides are columns 2, 3, 4 of the identity
__host__ __device__ constexpr int nlp_aaa_kind(int q) { return (q == 0 || q == 5) ? 1 : ((q == 1 || q == 6) ? 2 : 0); }
__host__ __device__ constexpr int nlp_aaa_which(int q) { return q < 3 ? 0 : (q == 3 ? 1 : 2); }

// row q from the powers of its plan time
__host__ __device__ __forceinline__ void nlp_aaa_row(int q, const double (&p)[7], double (&row)[7], double (&rr)[3]) {
  const int kind = nlp_aaa_kind(q);
  const double t = p[1], t2 = p[2], t3 = p[3], t4 = p[4], t5 = p[5], t6 = p[6];
  row[0] = kind == 0 ? t6 : (kind == 1 ? 6 * t5 : 30 * t4);
  row[1] = kind == 0 ? t5 : (kind == 1 ? 5 * t4 : 20 * t3);
  row[2] = kind == 0 ? t4 : (kind == 1 ? 4 * t3 : 12 * t2);
  row[3] = kind == 0 ? t3 : (kind == 1 ? 3 * t2 : 6 * t);
  row[4] = kind == 0 ? t2 : (kind == 1 ? 2 * t : 2.0);
  row[5] = kind == 0 ? t : (kind == 1 ? 1.0 : 0.0);
  row[6] = kind == 0 ? 1.0 : 0.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) rr[c] = (q == c + 2) ? 1.0 : 0.0;
}

// the whole system from the powers of the three plan times
__host__ __device__ __forceinline__ void nlp_aaa_fill(const double (&pw)[3][7], double (&m)[7][7], double (&r)[7][3]) {
#pragma unroll
  for (int q = 0; q < 7; ++q) nlp_aaa_row(q, pw[nlp_aaa_which(q)], m[q], r[q]);
}

// position, velocity and acceleration rows times the coefficients, in Eigen's order
__device__ __forceinline__ void nlp_poly(double t, const double (&co)[7], double &z, double &vz, double &az) {
  double pw[7];
  nlp_powers(t, pw);
  const double t2 = pw[2], t3 = pw[3], t4 = pw[4], t5 = pw[5], t6 = pw[6];
  z = (((((t6 * co[0] + t5 * co[1]) + t4 * co[2]) + t3 * co[3]) + t2 * co[4]) + t * co[5]) + 1.0 * co[6];
  vz = ((((((6 * t5) * co[0] + (5 * t4) * co[1]) + (4 * t3) * co[2]) + (3 * t2) * co[3]) + (2 * t) * co[4]) +
        1.0 * co[5]) + 0.0 * co[6];
  az = ((((((30 * t4) * co[0] + (20 * t3) * co[1]) + (12 * t2) * co[2]) + (6 * t) * co[3]) + 2.0 * co[4]) +
        0.0 * co[5]) + 0.0 * co[6];
}

// ---- dense record <-> workspace -------------------------------------------
// IDX::REC doubles per robot; IDX::at(ws, B, rb, d) is where value d of robot rb lives
template <int LEN>
struct NlpFieldMajor {
  static constexpr int REC = LEN;
  static __device__ __forceinline__ double *at(double *ws, int64_t B, int64_t rb, int d) {
    return ws + (int64_t)d * B + rb;
  }
};
struct NlpStepRecord {  // section 14: the ts / tx head is row-major
  static constexpr int REC = ST_REC;
  static __device__ __forceinline__ double *at(double *ws, int64_t B, int64_t rb, int d) {
    return d < 2 * NLP_NS ? ws + (int64_t)(d / NLP_NS) * B * NLP_NS + rb * NLP_NS + d % NLP_NS
                          : ws + 2 * B * NLP_NS + (int64_t)(d - 2 * NLP_NS) * B + rb;
  }
};
using NlpTickRecord = NlpFieldMajor<TK_REC>;
using NlpNodeRecord = NlpFieldMajor<ND_REC>;

// one thread per value
template <class IDX, bool SET>
__global__ __launch_bounds__(256) void nlp_record_copy_kernel(int64_t B, double *ws, double *state) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= B * IDX::REC) return;
  double *w = IDX::at(ws, B, t / IDX::REC, (int)(t % IDX::REC));
  if (SET)
    *w = state[t];
  else
    state[t] = *w;
}

// the body of every qloco_nlp*_get_state (SET = false) / _set_state (SET = true)
template <class IDX, bool SET>
inline int nlp_record_copy(int64_t batch, const void *workspace, const double *state, void *stream, const char *where) {
  if (batch <= 0 || batch > kNlpMaxBatch || !workspace || !state) return QLOCO_ERR_ARG;
  const int64_t n = batch * IDX::REC;
  hipLaunchKernelGGL((nlp_record_copy_kernel<IDX, SET>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, batch, (double *)workspace, (double *)state);
  QLOCO_HIP_CHECK(hipGetLastError(), where);
  return QLOCO_OK;
}

// ---- parameter checks: each layer adds its own to the one below -------------
inline bool nlp_params_ok(const qloco_nlp_params *p) {
  return p && p->dt > 0 && p->tstep > 0 && p->g > 0 && p->z_c > 0;
}

inline bool nlp_tick_params_ok(const qloco_nlp_params *p, const qloco_nlp_tick_params *tp) {
  if (!nlp_params_ok(p) || !tp || !(tp->hcom > 0)) return false;
  // the ring holds round(t_max / dt) ticks of a step, the two-tick look-back and the forecast slot
  const double n = round(p->t_max / p->dt);
  return n >= 0 && n + 4 <= TK_RING;
}

}  // namespace qloco

// qloco_srbd_core.hpp -- definitions shared by the SRBD kernel translation
// units (qloco_srbd.hip: the stance-only and two-wave / wide classes;
// qloco_srbd_lit.hip: the literal QP through the wrench space).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "qloco_common.hpp"
#include "qloco_dpp.inc"
#include "qloco_srbd_spec.hpp"

namespace qloco {

struct SrbdArgs {
  int N, feet_per_step, contacts_per_step, output_frame;
  float dt, mass;
  float inertia[9];
  float q2[13];  // 2 * q_weights (Q diagonal, ConvexMpc.cpp:18-24)
  float r2[12];  // 2 * r_weights (R diagonal, :38-45)
  float mu, fz_min, fz_max;
  float rho, sigma, alpha, eps_abs, eps_rel;
  int max_iter, check_termination, scaling, adaptive_rho, rho_interval;
  float rho_tol;
  int warm_start;
  // 1: the reference's full 12N-variable QP (every (step, leg) pair is a
  // variable; swing legs held by fz in [0, 0] rows), 0: stance-only reduction
  int literal;
  // instances with nlegs outside [leg_lo, leg_hi] belong to the other
  // launch of a split batch (qloco_srbd_solve_ex) and are skipped
  int leg_lo, leg_hi;
  int64_t batch;
  const float *x0, *xref, *feet;
  const uint8_t *contacts;
  float *u0, *u, *obj, *warm;
  int *status, *iters, *rho_updates;
  // optional instance list (positions 0..count-1 -> instance ids) and its
  // device-side length (qloco_srbd_solve_ex's class lists)
  const int *list;
  const int *count;
  // one-wave literal kernel, cold start: the caller's placement state
  // (qloco_srbd_place.hpp).  hint[b] takes instance b's iteration count;
  // workgroup p solves the instance of rank place_assign(p), at
  // order[place_position(rank)], once the state's ready word, at
  // hint[-kPlaceHeader], equals the batch.  NULL: workgroup p solves p.
  // place_simds: the SIMD count S of both maps, S < batch <= 4 S.
  int *hint;
  const int *order;
  int place_simds;
  // one-wave literal kernel: the G^-1 horizon tables of the spec, computed on
  // the host once per spec (qloco_srbd_tables.cpp) and carried in the kernel
  // arguments -- no launch, no allocation, no copy of their own, and a
  // captured launch keeps its copy.  lit_tables = 0: the kernel builds them
  // (anisotropic omega weights, the two-wave kernel, spec.reserved[0] & 1).
  int lit_tables;
  float lit_sq;   // 1 / sqrt(q_omega): S = Rz' / sqrt(q_omega)
  float lit_gmx;  // max diag G^-1
  alignas(16) float lit_gtab[kLitN * kLitN * 6];  // LitLds<1>::gtab's layout
  // per-instance bodies (qloco_srbd_solve_model): batch rows of 16 floats in
  // qloco_srbd_model's layout, or NULL: mass, inertia, mu and fz_* above.
  // Read through srbd_body (qloco_srbd_model.hpp) only.  Last, so that every
  // other field keeps its offset in the kernel-argument segment.
  const float *model;
};

// The fields a spec determines; the batch, the buffers and the launch's
// class limits are the caller's
inline void srbd_args_from_spec(const qloco_srbd_spec *spec, SrbdArgs *a) {
  a->N = spec->horizon;
  a->feet_per_step = spec->feet_per_step;
  a->contacts_per_step = spec->contacts_per_step;
  a->output_frame = spec->output_frame;
  a->dt = spec->dt;
  a->mass = spec->mass;
  for (int k = 0; k < 9; ++k) a->inertia[k] = spec->inertia[k];
  srbd_doubled_weights(spec, a->q2, a->r2);
  a->mu = spec->mu;
  a->fz_min = spec->fz_min;
  a->fz_max = spec->fz_max;
  a->rho = spec->rho;
  a->sigma = spec->sigma;
  a->alpha = spec->alpha;
  a->eps_abs = spec->eps_abs;
  a->eps_rel = spec->eps_rel;
  a->max_iter = spec->max_iter;
  a->check_termination = spec->check_termination;
  a->scaling = spec->scaling;
  a->adaptive_rho = spec->adaptive_rho;
  a->rho_interval = spec->adaptive_rho_interval;
  a->rho_tol = spec->adaptive_rho_tolerance;
  a->warm_start = spec->warm_start;
  a->literal = spec->literal_full_qp ? 1 : 0;
}

typedef float f2v __attribute__((ext_vector_type(2)));
typedef float f4v __attribute__((ext_vector_type(4)));

// One register row of K / K^-1; every index is static after unrolling, so
// SROA keeps it in VGPRs.
template <int W>
struct Row {
  float k[64 * W];
};
#define KE(K, c) ((K).k[(c)])

template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xF,
                                                            0xF, false));
}
// Compile-time loop over columns C..E-1 (the DPP control of a column's
// broadcast must be a constant expression).
template <int C, int E>
struct ColLoop {
  template <class F>
  static __device__ __forceinline__ void run(F &&f) {
    f(std::integral_constant<int, C>{});
    ColLoop<C + 1, E>::run(f);
  }
};
template <int E>
struct ColLoop<E, E> {
  template <class F>
  static __device__ __forceinline__ void run(F &&) {}
};
// Column c of a 60-vector read as one 16-byte chunk per lane (lane l holds
// elements 4(l % 16) .. +3): DPP row_newbcast:(c / 4) of component c % 4.
template <int C>
__device__ __forceinline__ float dpp_col(const f4v &d) {
  constexpr int e = C & 3;
  const float v = e == 0 ? d.x : (e == 1 ? d.y : (e == 2 ? d.z : d.w));
  return dpp<0x150 + (C >> 2)>(v);
}

// threadIdx.x through an opaque copy: index arithmetic on it is recomputed
// where the phase runs instead of hoisted to the kernel entry and kept live
// across the ADMM loop (at 128 VGPRs such hoisted offsets become spills)
__device__ __forceinline__ int opaque_tid() {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}

// The lane index regenerated by two VALU (mbcnt) where it is needed: a
// volatile asm is neither hoisted nor merged, so no VGPR carries the lane
// across a long phase (one-wave kernels only: lane == threadIdx.x there)
__device__ __forceinline__ int fresh_lane() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}

// a wave-uniform float held in an SGPR
__device__ __forceinline__ float sgpr_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

__device__ __forceinline__ float lane_prev(float v) { return dpp<0x138>(v); }  // wave_shr:1
__device__ __forceinline__ float lane_next(float v) { return dpp<0x130>(v); }  // wave_shl:1
__device__ __forceinline__ float rlane(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

// Wave-uniform max / sum over 64 lanes: DPP within 16-lane rows, then the
// four row results combined in a fixed order (deterministic).
__device__ __forceinline__ float wmax(float v) {
  v = fmaxf(v, dpp<0xB1>(v));   // quad_perm [1,0,3,2]
  v = fmaxf(v, dpp<0x4E>(v));   // quad_perm [2,3,0,1]
  v = fmaxf(v, dpp<0x124>(v));  // row_ror:4
  v = fmaxf(v, dpp<0x128>(v));  // row_ror:8
  return fmaxf(fmaxf(rlane(v, 0), rlane(v, 16)), fmaxf(rlane(v, 32), rlane(v, 48)));
}
__device__ __forceinline__ float wsum(float v) {
  v += dpp<0xB1>(v);
  v += dpp<0x4E>(v);
  v += dpp<0x124>(v);
  v += dpp<0x128>(v);
  return (rlane(v, 0) + rlane(v, 16)) + (rlane(v, 32) + rlane(v, 48));
}

// Block-wide reductions (wave-uniform results).
// Wave max of a NON-NEGATIVE float: the bits order like unsigned integers,
// so v_max_u32_dpp does each step in one op (no NaN canonicalisation): the
// four in-row steps, then row_bcast:15 / row_bcast:31 fold the rows into lane
// 63 (gfx9 DPP), read once.
#define QL_DMAXU(U, CTRL)                                                       \
  asm("s_nop 1\n\tv_max_u32_dpp %0, %0, %0 " CTRL " bank_mask:0xf" : "+v"(U))
__device__ __forceinline__ float wmax_nonneg(float v) {
  unsigned u = __builtin_bit_cast(unsigned, v);
  QL_DMAXU(u, "quad_perm:[1,0,3,2] row_mask:0xf");
  QL_DMAXU(u, "quad_perm:[2,3,0,1] row_mask:0xf");
  QL_DMAXU(u, "row_ror:4 row_mask:0xf");
  QL_DMAXU(u, "row_ror:8 row_mask:0xf");
  QL_DMAXU(u, "row_bcast:15 row_mask:0xa");  // rows 1, 3 += rows 0, 2
  QL_DMAXU(u, "row_bcast:31 row_mask:0xc");  // rows 2, 3 += lane 31
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(u, 63));
}

// Six such maxima at once, stage by stage: a chain's next step reads its
// register five instructions after the write, so the DPP read-after-write
// slots hold the other chains' steps and only the first stage is padded
// (six serial chains pay an s_nop per step).  Max is exact: the same values.
#define QL_DMAXU6(CTRL)                                      \
  "v_max_u32_dpp %0, %0, %0 " CTRL " bank_mask:0xf\n\t"      \
  "v_max_u32_dpp %1, %1, %1 " CTRL " bank_mask:0xf\n\t"      \
  "v_max_u32_dpp %2, %2, %2 " CTRL " bank_mask:0xf\n\t"      \
  "v_max_u32_dpp %3, %3, %3 " CTRL " bank_mask:0xf\n\t"      \
  "v_max_u32_dpp %4, %4, %4 " CTRL " bank_mask:0xf\n\t"      \
  "v_max_u32_dpp %5, %5, %5 " CTRL " bank_mask:0xf\n\t"
__device__ __forceinline__ void wmax_nonneg6(float (&v)[6]) {
  unsigned u[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) u[k] = __builtin_bit_cast(unsigned, v[k]);
  asm("s_nop 1\n\t"
      QL_DMAXU6("quad_perm:[1,0,3,2] row_mask:0xf")
      QL_DMAXU6("quad_perm:[2,3,0,1] row_mask:0xf")
      QL_DMAXU6("row_ror:4 row_mask:0xf")
      QL_DMAXU6("row_ror:8 row_mask:0xf")
      QL_DMAXU6("row_bcast:15 row_mask:0xa")
      QL_DMAXU6("row_bcast:31 row_mask:0xc")
      : "+v"(u[0]), "+v"(u[1]), "+v"(u[2]), "+v"(u[3]), "+v"(u[4]), "+v"(u[5]));
#pragma unroll
  for (int k = 0; k < 6; ++k) v[k] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(u[k], 63));
}

// K0 / K2 horizon sums (exact small integers in fp32).
__device__ __forceinline__ void k0k2(float ja, float jb, float Nf, float &K0, float &K2) {
  const float M = fmaxf(ja, jb);
  const float T = Nf - M;
  const float al = M - ja, be = M - jb;
  const float S1 = 0.5f * T * (T - 1.0f);
  const float S2 = rintf(S1 * (2.0f * T - 1.0f) * (1.0f / 3.0f));
  K0 = T;
  K2 = S2 + (al + be) * S1 + al * be * T;
}

// Gauss-Jordan: pivots above this get their column written exactly (qloco_srbd.hip)
constexpr float kGjExactPivot = 16.0f;

static_assert(sizeof(SrbdArgs) <= 4096, "kernel argument segment");
static_assert(offsetof(SrbdArgs, lit_gtab) % 16 == 0, "lit_gtab is read in 16-byte chunks");

// place: the caller's placement state or NULL; simds: spec.reserved[1]
// (0 = four per compute unit of the current device)
// a.model set: the instantiations that read the rows
int srbd_lit_launch(const SrbdArgs &a, bool warm, int32_t *place, int simds, hipStream_t stream);
int srbd_place_launch(int32_t *place, int64_t batch, int simds, int check_termination,
                      hipStream_t stream);

}  // namespace qloco

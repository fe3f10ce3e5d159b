// Element Gauss-Jordan of the one-wave literal SRBD kernel (lit_invert,
// qloco_srbd_lit.hip) with the per-pivot rank-1 update on the matrix cores:
// two v_mfma_f32_32x32x1_2b_f32 per pivot in place of 60 v_fmac_f32_dpp
// (DESIGN.md §3t).  Three measurements:
//   (a) the MFMA result against fmaf(a, b, c) per entry, bit for bit: random
//       operands, denormals, signed zeros, infinities, NaNs; and the C/D
//       (lane, register) <-> (row, column) map, read off the hardware
//   (b) issue cycles and dependent-accumulator latency of the instruction
//   (c) a 60-pivot inverse in the MFMA form against lit_invert's loop, same
//       60 x 60 SPD inputs, inverse compared byte for byte, timed at 1, 2 and
//       4 waves per SIMD
// Build: hipcc --offload-arch=gfx950 -O3 -I../../quadrupedal_loco_amd/csrc lit_mfma_gj.hip -o lit_mfma_gj
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include "qloco_dpp.inc"

typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f32x32 __attribute__((ext_vector_type(32)));

constexpr float kGjExactPivot = 16.0f;

#define HIP_OK(x)                                                         \
  do {                                                                    \
    hipError_t e_ = (x);                                                  \
    if (e_ != hipSuccess) {                                               \
      printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); \
      return 2;                                                           \
    }                                                                     \
  } while (0)

__device__ __forceinline__ void lsync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
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
template <int C>
__device__ __forceinline__ float dpp_col(const f4v &d) {
  constexpr int e = C & 3;
  const float v = e == 0 ? d.x : (e == 1 ? d.y : (e == 2 ? d.z : d.w));
  return dpp<0x150 + (C >> 2)>(v);
}
__device__ __forceinline__ float rlane(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

// The accumulator map of v_mfma_f32_32x32x1_2b_f32 (part (a) checks it on the
// hardware): D register r, lane l holds block r / 16, row
// (r & 3) + 8 ((r & 15) / 4) + 4 (l / 32), column l & 31, and that entry is
// fma(A[32 block + row], B[32 block + column], C).
__host__ __device__ constexpr int mfma_blk(int r) { return r >> 4; }
__host__ __device__ constexpr int mfma_row(int r, int l) { return (r & 3) + 8 * ((r & 15) >> 2) + 4 * (l >> 5); }
__host__ __device__ constexpr int mfma_col(int l) { return l & 31; }

// ---------------- (a) bits
__global__ __launch_bounds__(64) void mfma_bits(const float *a, const float *b, const float *c, float *d, float *dv) {
  const int l = threadIdx.x;
  const int64_t cs = blockIdx.x;
  const float av = a[cs * 64 + l], bv = b[cs * 64 + l];
  f32x32 acc;
#pragma unroll
  for (int r = 0; r < 32; ++r) acc[r] = c[(cs * 32 + r) * 64 + l];
  const f32x32 out = __builtin_amdgcn_mfma_f32_32x32x1f32(av, bv, acc, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 32; ++r) {
    d[(cs * 32 + r) * 64 + l] = out[r];
    const float ae = a[cs * 64 + 32 * mfma_blk(r) + mfma_row(r, l)], be = b[cs * 64 + 32 * mfma_blk(r) + mfma_col(l)];
    dv[(cs * 32 + r) * 64 + l] = __builtin_fmaf(ae, be, acc[r]);  // v_fma_f32
  }
}

// ---------------- (b) cycles.  out[0..5]: s_memtime and s_memrealtime (100 MHz) deltas
template <int MODE>  // 0: two independent accumulators, 1: one dependent chain, 2: chain through a VALU read of the result
__global__ __launch_bounds__(64) void mfma_cycles(float *sink, long long *out, int n) {
  const int l = threadIdx.x;
  float av = 1.0f + l * 1e-3f, bv = 1.0f - l * 1e-3f;
  f32x32 x, y;
#pragma unroll
  for (int r = 0; r < 32; ++r) x[r] = y[r] = 0.0f;
  const long long t0 = clock64(), w0 = wall_clock64();
  for (int i = 0; i < n; ++i) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if constexpr (MODE == 0) {
        x = __builtin_amdgcn_mfma_f32_32x32x1f32(av, bv, x, 0, 0, 0);
        y = __builtin_amdgcn_mfma_f32_32x32x1f32(av, bv, y, 0, 0, 0);
      } else if constexpr (MODE == 1) {
        x = __builtin_amdgcn_mfma_f32_32x32x1f32(av, bv, x, 0, 0, 0);
        x = __builtin_amdgcn_mfma_f32_32x32x1f32(av, bv, x, 0, 0, 0);
      } else {
        x = __builtin_amdgcn_mfma_f32_32x32x1f32(av, bv, x, 0, 0, 0);
        av = x[31] * 1e-30f;  // the last register written feeds the next A operand
        x = __builtin_amdgcn_mfma_f32_32x32x1f32(av, bv, x, 0, 0, 0);
        av = x[31] * 1e-30f;
      }
    }
  }
  const long long t1 = clock64(), w1 = wall_clock64();
  float s = av;
#pragma unroll
  for (int r = 0; r < 32; ++r) s += x[r] + y[r];
  sink[blockIdx.x * 64 + l] = s;
  if (l == 0 && blockIdx.x == 0) {
    out[0] = t1 - t0;
    out[1] = w1 - w0;
  }
}

// ---------------- (c) lit_invert's loop, as the kernel has it
template <int WPE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WPE, WPE)))
void gj_dpp(const float *in, float *out, int nm, int ncol, int reps) {
  __shared__ __attribute__((aligned(16))) f4v bc[16];
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  float K[64];
#pragma unroll
  for (int c = 0; c < 64; ++c) K[c] = in[(b % nm) * 4096 + lane * 64 + c];
  for (int rep = 0; rep < reps; ++rep) {
    int nc = __builtin_amdgcn_readfirstlane(ncol);
    {
      const float v = K[0];
      const float p = rlane(v, 0);
      reinterpret_cast<float *>(&bc[0])[lane] = lane == 0 ? p + 1.0f : v;
    }
    ColLoop<0, 60>::run([&](auto kc) {
      constexpr int k = decltype(kc)::value;
      asm volatile("" : "+s"(nc));
      if (k >= nc) return;
      const bool is_k = __builtin_amdgcn_inverse_ballot_w64(1ull << k);
      lsync();
      const f4v r0 = bc[lane & 15];
      const float v = K[k];
      const float p = rlane(v, k);
      const float pinv = __builtin_amdgcn_rcpf(p);
      const float ng = is_k ? pinv - 1.0f : -v * pinv;
      if constexpr (k + 1 < 60) {
        const bool is_k1 = __builtin_amdgcn_inverse_ballot_w64(1ull << (k + 1));
        const bool upto_k = __builtin_amdgcn_inverse_ballot_w64((2ull << k) - 1ull);
        const float la = fmaf(dpp_col<k + 1>(r0), ng, K[k + 1]);
        const float p1 = rlane(la, k + 1);
        reinterpret_cast<float *>(&bc[0])[lane] = is_k1 ? p1 + 1.0f : (upto_k ? -la : la);
      }
      QL_DPP_GJ60_P1(K, 0, r0, ng);
      if (p > kGjExactPivot) K[k] = is_k ? pinv : ng;
    });
    lsync();
  }
#pragma unroll
  for (int c = 0; c < 64; ++c) out[b * 4096 + lane * 64 + c] = K[c];
}

// ---------------- (c) the MFMA form
//
// Row layout: lane i, register j holds K[i][j].  Accumulator layout: four
// 32 x 32 blocks (jb, ib) = (j / 32, i / 32); block (jb, ib)'s register q,
// lane l holds K[32 ib + (l & 31)][32 jb + mfma_row(q, l)] -- the MFMA row is
// the column index j, the MFMA column (the lane) the row index i.  With
// j0(q) = (q & 3) + 8 (q / 4), one v_permlane32_swap of row registers
// 32 jb + j0 and 32 jb + j0 + 4 leaves block (jb, 0)'s register q in the first
// and block (jb, 1)'s in the second; the same swap converts back.
__device__ __forceinline__ void swap32(float &a, float &b) {
  const auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b), false, false);
  // (elements copied out first: __builtin_bit_cast of the vector element
  // r[1] itself reads element 0 with this compiler)
  const unsigned r0 = r[0], r1 = r[1];
  a = __builtin_bit_cast(float, r0);  // (a.lo, b.lo)
  b = __builtin_bit_cast(float, r1);  // (a.hi, b.hi)
}
__host__ __device__ constexpr int gj_j0(int q) { return (q & 3) + 8 * (q >> 2); }

// D1: blocks (0, 0) and (1, 1); D2: blocks (0, 1) and (1, 0)
__device__ __forceinline__ void gj_to_acc(const float (&K)[64], f32x32 &D1, f32x32 &D2) {
#pragma unroll
  for (int jb = 0; jb < 2; ++jb)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      float a = K[32 * jb + gj_j0(q)], b = K[32 * jb + gj_j0(q) + 4];
      swap32(a, b);  // a: block (jb, 0), b: block (jb, 1)
      if (jb == 0) {
        D1[q] = a;
        D2[q] = b;
      } else {
        D2[16 + q] = a;
        D1[16 + q] = b;
      }
    }
}
__device__ __forceinline__ void gj_from_acc(float (&K)[64], const f32x32 &D1, const f32x32 &D2) {
#pragma unroll
  for (int jb = 0; jb < 2; ++jb)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      float a = jb == 0 ? D1[q] : D2[16 + q], b = jb == 0 ? D2[q] : D1[16 + q];
      swap32(a, b);
      K[32 * jb + gj_j0(q)] = a;
      K[32 * jb + gj_j0(q) + 4] = b;
    }
}

template <int k>
__device__ __forceinline__ void gj_mfma_pivot(f32x32 &D1, f32x32 &D2) {
  constexpr int jb = k >> 5, kk = k & 31, h = (kk >> 2) & 1, q = (kk & 3) + 4 * (kk >> 3);
  static_assert(gj_j0(q) + 4 * h == kk, "column k is register q of the blocks (jb, .), lane half h");
  constexpr int x1 = jb == 0 ? q : 16 + q;  // block (jb, 0): D1 for jb = 0, D2 for jb = 1; block (jb, 1) the other
  const bool is_k = __builtin_amdgcn_inverse_ballot_w64(1ull << k);
  const bool is_ks = __builtin_amdgcn_inverse_ballot_w64(1ull << (k ^ 32));
  const bool before_k = __builtin_amdgcn_inverse_ballot_w64((1ull << k) - 1ull);
  const bool lo = __builtin_amdgcn_inverse_ballot_w64(0xffffffffull);
  // column k of every row as a 64-lane vector: rows < 32 from block (jb, 0),
  // rows >= 32 from block (jb, 1), both in lane half h
  float X = jb == 0 ? D1[x1] : D2[x1], Y = jb == 0 ? D2[x1] : D1[x1];
  swap32(X, Y);
  const float v = h == 0 ? X : Y;
  const float p = rlane(v, k);
  const float pinv = __builtin_amdgcn_rcpf(p);
  const float ng = is_k ? pinv - 1.0f : -v * pinv;
  const float c = is_k ? p + 1.0f : (before_k ? -v : v);
  float nl = ng, nh = ng;
  swap32(nl, nh);                    // (ng.lo, ng.lo), (ng.hi, ng.hi)
  const float ngs = lo ? nh : nl;    // ng with its halves exchanged
  D1 = __builtin_amdgcn_mfma_f32_32x32x1f32(c, ng, D1, 0, 0, 0);
  D2 = __builtin_amdgcn_mfma_f32_32x32x1f32(c, ngs, D2, 0, 0, 0);
  if (p > kGjExactPivot) {  // column k exactly
    const bool half_h = h == 0 ? lo : !lo;
    const float e = is_k ? pinv : ng, es = is_ks ? pinv : ngs;
    // block (jb, 0) holds rows < 32 in half h: e for h = 0, es for h = 1; block (jb, 1) the other
    const float e0 = h == 0 ? e : es, e1 = h == 0 ? es : e;
    if constexpr (jb == 0) {
      D1[x1] = half_h ? e0 : D1[x1];
      D2[x1] = half_h ? e1 : D2[x1];
    } else {
      D2[x1] = half_h ? e0 : D2[x1];
      D1[x1] = half_h ? e1 : D1[x1];
    }
  }
}

template <int WPE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WPE, WPE)))
void gj_mfma(const float *in, float *out, int nm, int ncol, int reps) {
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  float K[64];
#pragma unroll
  for (int c = 0; c < 64; ++c) K[c] = in[(b % nm) * 4096 + lane * 64 + c];
  for (int rep = 0; rep < reps; ++rep) {
    int nc = __builtin_amdgcn_readfirstlane(ncol);
    f32x32 D1, D2;
    gj_to_acc(K, D1, D2);
    ColLoop<0, 60>::run([&](auto kc) {
      constexpr int k = decltype(kc)::value;
      asm volatile("" : "+s"(nc));
      if (k >= nc) return;
      gj_mfma_pivot<k>(D1, D2);
    });
    gj_from_acc(K, D1, D2);
  }
#pragma unroll
  for (int c = 0; c < 64; ++c) out[b * 4096 + lane * 64 + c] = K[c];
}

// ---------------- host
static uint32_t bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
static float fbits(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}
static uint32_t rng_s = 2463534242u;
static uint32_t rnd32() {
  rng_s ^= rng_s << 13;
  rng_s ^= rng_s >> 17;
  rng_s ^= rng_s << 5;
  return rng_s;
}
static float rnd_unit() { return (float)((rnd32() >> 8) / 16777216.0 * 2.0 - 1.0); }
static float rnd_denorm() { return fbits((rnd32() & 0x807fffffu)); }
static float rnd_any_finite() {
  uint32_t u;
  do u = rnd32();
  while (((u >> 23) & 0xff) == 0xff);
  return fbits(u);
}

struct CaseSet {
  const char *name;
  int first, count;
};

static int part_a(FILE *f) {
  // case sets: fill a[64], b[64], c[32][64] per case
  const int PER = 48;
  std::vector<CaseSet> sets;
  std::vector<float> a, b, c;
  auto add_set = [&](const char *name, auto gen) {
    sets.push_back({name, (int)(a.size() / 64), PER});
    for (int cs = 0; cs < PER; ++cs) {
      for (int i = 0; i < 64; ++i) {
        a.push_back(gen(0));
        b.push_back(gen(1));
      }
      for (int i = 0; i < 2048; ++i) c.push_back(gen(2));
    }
  };
  add_set("random in [-1, 1)", [](int) { return rnd_unit(); });
  add_set("random finite bit patterns (any exponent)", [](int) { return rnd_any_finite(); });
  add_set("denormal a, b, c", [](int) { return rnd_denorm(); });
  add_set("denormal a; b, c in [-1, 1)", [](int w) { return w == 0 ? rnd_denorm() : rnd_unit(); });
  add_set("a, b in [-1, 1) x 2^-70 (denormal products); c denormal",
          [](int w) { return w == 2 ? rnd_denorm() : rnd_unit() * 0x1p-70f; });
  add_set("a, b in [-1, 1) x 2^-63; c in [-1, 1) x 2^-126 (denormal results)",
          [](int w) { return w == 2 ? rnd_unit() * 0x1p-126f : rnd_unit() * 0x1p-63f; });
  add_set("signed zeros among [-1, 1)", [](int) {
    const uint32_t r = rnd32() % 6;
    return r == 0 ? 0.0f : (r == 1 ? -0.0f : rnd_unit());
  });
  add_set("all signed zeros", [](int) { return (rnd32() & 1) ? 0.0f : -0.0f; });
  add_set("infinities among [-1, 1) and zeros", [](int) {
    const uint32_t r = rnd32() % 8;
    return r == 0 ? INFINITY : (r == 1 ? -INFINITY : (r == 2 ? 0.0f : rnd_unit()));
  });
  add_set("NaNs (quiet, signalling, payloads) among [-1, 1)", [](int) {
    const uint32_t r = rnd32() % 8;
    return r == 0 ? fbits(0x7fc00000u | (rnd32() & 0x3fffffu)) : (r == 1 ? fbits(0xff800001u | (rnd32() & 0x3fffffu)) : rnd_unit());
  });
  const int NC = (int)(a.size() / 64);
  float *da, *db, *dc, *dd, *dv;
  HIP_OK(hipMalloc(&da, a.size() * 4));
  HIP_OK(hipMalloc(&db, b.size() * 4));
  HIP_OK(hipMalloc(&dc, c.size() * 4));
  HIP_OK(hipMalloc(&dd, c.size() * 4));
  HIP_OK(hipMalloc(&dv, c.size() * 4));
  HIP_OK(hipMemcpy(da, a.data(), a.size() * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(db, b.data(), b.size() * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(dc, c.data(), c.size() * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(mfma_bits, dim3(NC), dim3(64), 0, 0, da, db, dc, dd, dv);
  HIP_OK(hipDeviceSynchronize());
  std::vector<float> d(c.size()), v(c.size());
  HIP_OK(hipMemcpy(d.data(), dd, d.size() * 4, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(v.data(), dv, v.size() * 4, hipMemcpyDeviceToHost));
  fprintf(f, "(a) v_mfma_f32_32x32x1_2b_f32 against fmaf(a, b, c) per entry, %d cases x 2048 entries per set\n", PER);
  fprintf(f, "    map under test: D register r, lane l = block r/16, row (r&3) + 8((r&15)/4) + 4(l/32), column l&31\n");
  fprintf(f, "    columns: entries | != v_fma_f32 on the device | != host fmaf | of those, both NaN (payload or sign only)\n");
  int finite_bad = 0;
  for (const CaseSet &s : sets) {
    long n = 0, bad_v = 0, bad_h = 0, bad_v_nan = 0, bad_h_nan = 0;
    for (int cs = s.first; cs < s.first + s.count; ++cs)
      for (int r = 0; r < 32; ++r)
        for (int l = 0; l < 64; ++l) {
          const size_t idx = ((size_t)cs * 32 + r) * 64 + l;
          const float ae = a[(size_t)cs * 64 + 32 * mfma_blk(r) + mfma_row(r, l)];
          const float be = b[(size_t)cs * 64 + 32 * mfma_blk(r) + mfma_col(l)];
          const float hf = fmaf(ae, be, c[idx]);
          ++n;
          if (bits(d[idx]) != bits(v[idx])) {
            ++bad_v;
            if (std::isnan(d[idx]) && std::isnan(v[idx])) ++bad_v_nan;
          }
          if (bits(d[idx]) != bits(hf)) {
            ++bad_h;
            if (std::isnan(d[idx]) && std::isnan(hf)) ++bad_h_nan;
          }
        }
    fprintf(f, "    %-62s %7ld | %6ld (%ld NaN) | %6ld (%ld NaN)\n", s.name, n, bad_v, bad_v_nan, bad_h, bad_h_nan);
    const bool finite_set = &s - sets.data() < 8;
    if (finite_set) finite_bad += (int)(bad_v + bad_h);
  }
  fprintf(f, "    finite operands (first eight sets): %s\n", finite_bad == 0 ? "BITWISE equal" : "NOT bitwise");
  hipFree(da), hipFree(db), hipFree(dc), hipFree(dd), hipFree(dv);
  return finite_bad == 0 ? 0 : 1;
}

static int part_b(FILE *f) {
  float *sink;
  long long *out;
  HIP_OK(hipMalloc(&sink, 1024 * 64 * 4));
  HIP_OK(hipMalloc(&out, 64));
  const int n = 2000;  // x 8 MFMAs
  fprintf(f, "(b) v_mfma_f32_32x32x1_2b_f32 cycles, one wave per SIMD (1024 workgroups of 64), %d instructions\n", 8 * n);
  const char *names[3] = {"two independent accumulators (issue)", "one accumulator (dependent chain)",
                          "one accumulator, A operand from a v_mul of the result"};
  for (int mode = 0; mode < 3; ++mode) {
    long long h[2] = {0, 0};
    for (int pass = 0; pass < 2; ++pass) {
      if (mode == 0) hipLaunchKernelGGL(mfma_cycles<0>, dim3(1024), dim3(64), 0, 0, sink, out, n);
      if (mode == 1) hipLaunchKernelGGL(mfma_cycles<1>, dim3(1024), dim3(64), 0, 0, sink, out, n);
      if (mode == 2) hipLaunchKernelGGL(mfma_cycles<2>, dim3(1024), dim3(64), 0, 0, sink, out, n);
      HIP_OK(hipDeviceSynchronize());
    }
    hipEvent_t e0, e1;
    hipEventCreate(&e0), hipEventCreate(&e1);
    hipEventRecord(e0);
    if (mode == 0) hipLaunchKernelGGL(mfma_cycles<0>, dim3(1024), dim3(64), 0, 0, sink, out, n);
    if (mode == 1) hipLaunchKernelGGL(mfma_cycles<1>, dim3(1024), dim3(64), 0, 0, sink, out, n);
    if (mode == 2) hipLaunchKernelGGL(mfma_cycles<2>, dim3(1024), dim3(64), 0, 0, sink, out, n);
    hipEventRecord(e1);
    HIP_OK(hipEventSynchronize(e1));
    float ms;
    hipEventElapsedTime(&ms, e0, e1);
    HIP_OK(hipMemcpy(h, out, 16, hipMemcpyDeviceToHost));
    fprintf(f, "    %-56s s_memtime %.1f / instr, s_memrealtime %.2f ns / instr, kernel %.2f ns / instr (%.1f cycles at 2.4 GHz)\n",
            names[mode], (double)h[0] / (8.0 * n), (double)h[1] * 10.0 / (8.0 * n), ms * 1e6 / (8.0 * n),
            ms * 1e6 / (8.0 * n) * 2.4);
  }
  hipFree(sink), hipFree(out);
  return 0;
}

template <int WPE>
static void launch_c(int form, int B, const float *dA, float *dO, int nm, int nc, int reps) {
  if (form == 0)
    hipLaunchKernelGGL(gj_dpp<WPE>, dim3(B), dim3(64), 0, 0, dA, dO, nm, nc, reps);
  else
    hipLaunchKernelGGL(gj_mfma<WPE>, dim3(B), dim3(64), 0, 0, dA, dO, nm, nc, reps);
}

static int part_c(FILE *f, int *faster4, int *slower1) {
  const int NM = 256, n = 60;
  std::vector<float> hA((size_t)NM * 4096, 0.0f);
  for (int m = 0; m < NM; ++m) {
    // SPD B B' / n + small diagonal, scaled to a maximal diagonal of about 1
    // (lit_invert's input is M / (a bound on max diag M)); rows and columns
    // 60 .. 63 are zero padding as in the kernel
    std::vector<double> Bm(n * n), A(n * n);
    for (auto &x : Bm) x = rnd_unit();
    double dmax = 0;
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        double acc = 0;
        for (int q = 0; q < n; ++q) acc += Bm[i * n + q] * Bm[j * n + q];
        A[i * n + j] = acc / n + (i == j ? 0.02 : 0.0);
        if (i == j) dmax = fmax(dmax, A[i * n + j]);
      }
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) hA[(size_t)m * 4096 + i * 64 + j] = (float)(A[i * n + j] / dmax);
    // not bitwise symmetric, like the kernel's M (its rows are rounded one by one)
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < i; ++j)
        if ((rnd32() & 3) == 0) hA[(size_t)m * 4096 + i * 64 + j] = nextafterf(hA[(size_t)m * 4096 + i * 64 + j], 2.0f);
  }
  float *dA, *dO;
  const int BMAX = 4096;
  HIP_OK(hipMalloc(&dA, hA.size() * 4));
  HIP_OK(hipMalloc(&dO, (size_t)BMAX * 4096 * 4));
  HIP_OK(hipMemcpy(dA, hA.data(), hA.size() * 4, hipMemcpyHostToDevice));
  std::vector<float> o0((size_t)NM * 4096), o1((size_t)NM * 4096);
  fprintf(f, "(c) 60-pivot inverse: lit_invert's DPP loop against the MFMA form (row layout in and out, conversions included)\n");
  for (int nc : {60, 36, 30, 18, 6}) {
    launch_c<4>(0, NM, dA, dO, NM, nc, 1);
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(o0.data(), dO, o0.size() * 4, hipMemcpyDeviceToHost));
    launch_c<4>(1, NM, dA, dO, NM, nc, 1);
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(o1.data(), dO, o1.size() * 4, hipMemcpyDeviceToHost));
    long diff = 0, big = 0;
    for (int m = 0; m < NM; ++m)
      for (int i = 0; i < 60; ++i)
        for (int j = 0; j < 60; ++j) {
          const size_t idx = (size_t)m * 4096 + i * 64 + j;
          if (bits(o0[idx]) != bits(o1[idx])) ++diff;
          if (fabsf(o0[idx]) > kGjExactPivot) ++big;
        }
    // the inverse against the input (nc = 60 only): max |A X - I|
    double res = 0;
    if (nc == 60)
      for (int m = 0; m < 4; ++m)
        for (int i = 0; i < 60; ++i)
          for (int j = 0; j < 60; ++j) {
            double acc = 0;
            for (int q = 0; q < 60; ++q) acc += (double)hA[(size_t)m * 4096 + i * 64 + q] * o1[(size_t)m * 4096 + q * 64 + j];
            res = fmax(res, fabs(acc - (i == j ? 1.0 : 0.0)));
          }
    fprintf(f, "    nc = %2d: %d matrices, %ld of %d entries differ in bits (entries above the exact-pivot bound %g: %ld)%s\n", nc,
            NM, diff, NM * 3600, (double)kGjExactPivot, big, nc == 60 ? "" : "");
    if (nc == 60) fprintf(f, "             max |A X - I| of the MFMA form's inverse, 4 matrices: %.3e\n", res);
    if (diff) {
      fprintf(f, "    NOT byte-identical: stop\n");
      return 1;
    }
  }
  // Two compilations: the register budget of four waves per SIMD at every load
  // (what the product kernel is compiled for: <= 128 VGPRs, the accumulators
  // updated in place), and the budget of the load itself (at one wave per SIMD
  // the compiler takes 140 VGPRs and another schedule).
  const int reps = 20;
  double us[2][3];
  for (int own = 0; own < 2; ++own) {
    fprintf(f, "    compiled for %s:\n", own ? "the load's own waves per SIMD" : "four waves per SIMD (as the kernel is)");
    for (int wi = 0; wi < 3; ++wi) {
      const int w = 1 << wi, B = 1024 * w;
      double t[2];
      for (int form = 0; form < 2; ++form) {
        float best = 1e30f;
        for (int pass = 0; pass < 4; ++pass) {
          hipEvent_t e0, e1;
          hipEventCreate(&e0), hipEventCreate(&e1);
          hipEventRecord(e0);
          if (own && w == 1) launch_c<1>(form, B, dA, dO, NM, 60, reps);
          if (own && w == 2) launch_c<2>(form, B, dA, dO, NM, 60, reps);
          if (!own || w == 4) launch_c<4>(form, B, dA, dO, NM, 60, reps);
          hipEventRecord(e1);
          HIP_OK(hipEventSynchronize(e1));
          float ms;
          hipEventElapsedTime(&ms, e0, e1);
          if (pass) best = fminf(best, ms);
        }
        t[form] = best * 1e3 / reps;
        if (!own) us[form][wi] = t[form];
      }
      fprintf(f, "      %d wave(s) per SIMD (B = %4d, %d inverses per wave): DPP %7.2f us, MFMA %7.2f us per inverse round  (%.0f / %.0f cycles per pivot round at 2.4 GHz)\n",
              w, B, reps, t[0], t[1], t[0] * 2400.0 / 60.0, t[1] * 2400.0 / 60.0);
    }
  }
  *faster4 = us[1][2] < us[0][2];
  *slower1 = us[1][0] > us[0][0];
  hipFree(dA), hipFree(dO);
  return 0;
}

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "w") : stdout;
  if (!f) return 2;
  hipDeviceProp_t prop;
  HIP_OK(hipGetDeviceProperties(&prop, 0));
  fprintf(f, "lit_mfma_gj probe on %s (%s), %d CUs\n", prop.name, prop.gcnArchName, prop.multiProcessorCount);
  const int ra = part_a(f);
  fflush(f);
  if (ra == 2) return 2;
  if (part_b(f)) return 2;
  fflush(f);
  int faster4 = 0, slower1 = 0;
  const int rc = part_c(f, &faster4, &slower1);
  if (rc == 2) return 2;
  fprintf(f, "verdict: (a) %s on finite operands; (c) %s; MFMA form %s at four waves per SIMD, %s at one\n",
          ra == 0 ? "bitwise" : "NOT bitwise", rc == 0 ? "byte-identical inverses" : "inverses differ",
          faster4 ? "faster" : "not faster", slower1 ? "slower" : "not slower");
  if (f != stdout) fclose(f);
  return (ra || rc) ? 1 : 0;
}

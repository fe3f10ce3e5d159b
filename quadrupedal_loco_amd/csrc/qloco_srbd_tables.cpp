// qloco_srbd_tables.cpp -- the literal QP's G^-1 horizon tables, once per
// spec on the host instead of once per instance in the kernel.
//
// G = K0 (x) Qb + K2 (x) Te splits by wrench component into six N x N blocks
// A_a = alpha_a K0 + beta_a K2 (qloco_srbd_lit.hip, "G^-1 in six N x N
// blocks").  For the v axes and omega_z, alpha and beta are weights and dt^2.
// For the omega x / y pair they carry the eigenvalues of Q^-1/2 T Q^-1/2,
// T = [Rz' diag(q_theta) Rz]_xy: with q_omega_x = q_omega_y = q that matrix
// is Rz' diag(q_theta) Rz / q, a similarity of diag(q_theta) / q -- the
// eigenvalues (q_theta_x, q_theta_y) / q hold for every yaw and the
// eigenvectors are the columns of Rz', so S = Rz' / sqrt(q) is the only
// per-instance part (two multiplies from the model's cos / sin).
//
// Same operation sequence as the kernel's float64 block -- explicit fma,
// correctly rounded divides, the lock-step Gauss-Jordan's update order -- and
// this unit is compiled without FMA contraction, so the yaw-independent axes
// (omega_z, v) are bit-identical to the kernel's tables.  The eigen axes
// match the kernel's at yaw = 0; at other yaws its Jacobi rotation leaves a
// float64 rounding in lambda, at most one float32 ulp in a table entry.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <mutex>

#include "qloco.h"
#include "qloco_srbd_spec.hpp"
#include "qloco_srbd_tables.hpp"

namespace qloco {

bool srbd_lit_tables_host(int N, float dt, const float *q2, float *gtab, float *sq, float *gmx) {
  if (N < 1 || N > kLitN2) return false;
  if (!(q2[6] > 0.0f) || q2[6] != q2[7]) return false;
  const int NT = N <= kLitN ? kLitN : kLitN2;
  const int H = N <= kLitN ? N : (N + 1) / 2;
  const double dt2 = (double)dt * (double)dt;
  const double ix = 1.0 / sqrt((double)q2[6]);
  const double lam[2] = {(double)q2[0] * ix * ix, (double)q2[1] * ix * ix};
  memset(gtab, 0, sizeof(float) * NT * NT * 6);
  float dmax = 0.0f;
  for (int ax = 0; ax < 6; ++ax) {
    const double al = ax < 2 ? 1.0 : (ax == 2 ? (double)q2[8] : (double)q2[9 + ax - 3]);
    const double be = ax < 2 ? dt2 * lam[ax] : dt2 * (double)q2[ax];  // q_theta_z / q_p: q2[2..5]
    const double sn2 = ax < 2 ? ix * ix : 1.0;  // |S column|^2 (the gmx bound)
    double A[kLitN2][kLitN2];
    for (int ri = 0; ri < N; ++ri)
      for (int k = 0; k < N; ++k) {
        const int M = ri > k ? ri : k;
        const double T0 = (double)(N - M), ia = (double)(M - ri), ib = (double)(M - k);
        const double S1 = 0.5 * T0 * (T0 - 1.0), S2 = (T0 - 1.0) * T0 * (2.0 * T0 - 1.0) / 6.0;
        const double K2 = S2 + (ia + ib) * S1 + ia * ib * T0;
        A[ri][k] = fma(al, T0, be * K2);
      }
    // in-place Gauss-Jordan, every row against the pivot row as it stood
    // before the pivot (the kernel's lanes read it from an LDS copy)
    for (int k = 0; k < N; ++k) {
      double pr[kLitN2];
      for (int c = 0; c < N; ++c) pr[c] = A[k][c];
      const double pinv = 1.0 / pr[k];
      for (int ri = 0; ri < N; ++ri) {
        double *row = A[ri];
        const double fk = row[k] * pinv;
        for (int c = 0; c < N; ++c) {
          if (c == k) continue;
          row[c] = ri == k ? pr[c] * pinv : fma(-fk, pr[c], row[c]);
        }
        row[k] = ri == k ? pinv : -fk;
      }
    }
    for (int ri = 0; ri < N; ++ri) {
      const int csi = ri < H ? ri : kLitN + ri - H;
      for (int k = 0; k < N; ++k) {
        const int csk = k < H ? k : kLitN + k - H;
        gtab[(csi * NT + csk) * 6 + ax] = (float)A[ri][k];
      }
      dmax = fmaxf(dmax, (float)(sn2 * A[ri][ri]));
    }
  }
  *sq = (float)ix;
  *gmx = dmax;
  return true;
}

namespace {
struct TabEntry {
  bool used = false;
  int N = 0;
  float dt = 0.0f, q2[12] = {}, sq = 0.0f, gmx = 0.0f;
  float gtab[kLitN * kLitN * 6] = {};
};
constexpr int kTabEntries = 8;
std::mutex g_tab_mu;
TabEntry g_tab[kTabEntries];
int g_tab_next = 0;
}  // namespace

bool srbd_lit_tables_cached(int N, float dt, const float *q2, float *gtab, float *sq, float *gmx) {
  if (N < 1 || N > kLitN) return false;
  if (!(q2[6] > 0.0f) || q2[6] != q2[7]) return false;
  std::lock_guard<std::mutex> lk(g_tab_mu);
  TabEntry *e = nullptr;
  for (int i = 0; i < kTabEntries && !e; ++i)
    if (g_tab[i].used && g_tab[i].N == N && memcmp(&g_tab[i].dt, &dt, sizeof(dt)) == 0 &&
        memcmp(g_tab[i].q2, q2, sizeof(g_tab[i].q2)) == 0)
      e = &g_tab[i];
  if (!e) {
    e = &g_tab[g_tab_next];
    g_tab_next = (g_tab_next + 1) % kTabEntries;
    e->used = false;
    if (!srbd_lit_tables_host(N, dt, q2, e->gtab, &e->sq, &e->gmx)) return false;
    e->N = N;
    e->dt = dt;
    memcpy(e->q2, q2, sizeof(e->q2));
    e->used = true;
  }
  memcpy(gtab, e->gtab, sizeof(e->gtab));
  *sq = e->sq;
  *gmx = e->gmx;
  return true;
}

}  // namespace qloco

extern "C" int qloco_srbd_lit_tables(const qloco_srbd_spec *spec, float *gtab, int64_t gtab_len,
                                     float *s_scale, float *gmx, int32_t *served) {
  if (!spec || !gtab || !s_scale || !gmx || !served) return QLOCO_ERR_ARG;
  const int N = spec->horizon;
  if (N < 1 || N > qloco::kLitN2) return QLOCO_BAD_SIZE;
  const int NT = N <= qloco::kLitN ? qloco::kLitN : qloco::kLitN2;
  if (gtab_len < (int64_t)NT * NT * 6) return QLOCO_ERR_ARG;
  float q2[13];
  qloco::srbd_doubled_weights(spec, q2, nullptr);
  *served = qloco::srbd_lit_tables_host(N, spec->dt, q2, gtab, s_scale, gmx) ? 1 : 0;
  return QLOCO_OK;
}

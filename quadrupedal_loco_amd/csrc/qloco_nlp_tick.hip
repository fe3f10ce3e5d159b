// qloco_nlp_tick.hip -- the rest of the slow planner's tick, batched (fp64,
// gfx950): CoM height, ZMP / DCM and the swing feet.
//
// qloco_nlp_tick launches the step-timing kernel of qloco_nlp.hip unchanged
// (through qloco_nlp_step_timing) and then, on the same stream, one kernel
// that adds what NLPClass::step_timing_opti_loop and
// Foot_trajectory_solve_mod2 compute around the SQP
// (unitree_ros/mosek_nlp_kmp/src/NLP/NLPClass_sqp.cpp; line numbers below are
// that file's): CoM_height_solve (:2361-2473) as :936 calls it, with the
// _bjx1 of the previous tick; the ZMP / DCM samples (:950-954) with _Zsc of
// Initialize (:323-328); the 38-vector (:1048-1090); the swing feet
// (:2039-2358) with solve_AAA_inv2 (:3633-3644).  tests/nlp_tick_ref.py is the
// line-by-line restatement (compile with -ffp-contract=off).  CoM_height_solve
// keeps the operation order of its formulation A: the LU inverse, then the
// product, with powers formed correctly rounded, as pow() returns them.  The
// swing foot's 4 x 4 system does not: it is solved by pivoted LU (formulation
// B's algebra, powers by multiplication), because the cofactor inverse that
// formulation A transcribes turns a one-ulp change of _ts into 1e-13 .. 1e-12 m
// on well-conditioned ticks, and the device SQP's _ts is
// not the restatement's to the ulp.  The polynomials are evaluated in A's order.
//
// Two forms with identical bits.  Shipped: one robot per lane; the 7 x 7 system
// is factorised by a fully unrolled partial-pivot LU whose pivot search and
// row swaps are compares and selects, so the matrix stays in registers.  A/B:
// one robot per 8-lane group with a matrix row per lane and cross-lane moves
// (qloco_nlp_tick_set_group_width).  Only the three columns of the inverse
// that meet a non-zero of comz_plan are formed.
//
// Second workspace (doubles), field-major, the TK_ offsets of
// qloco_nlp_core.hpp: previous _bjx1 | _ry_left_right | _t_end_footstep |
// _stepwidth(0) | the last tick index | _footz_ref[27] | _lift_height_ref[27] |
// the initial _tx[27] | a ring of (Rfoot xyz, Lfoot xyz), array index k in
// entry k % RING; then the step-timing kernel's scratch.  The powers, the LU
// and the bounded reads are that header's too.  The fill of AAA, the
// polynomial and the _Zsc search are written out here in the order the kernel
// was tuned in: calling the header's nlp_aaa_fill / nlp_poly instead gives the
// same bits in another schedule (profiles/nlp_core_ab.txt).
#include <atomic>
#include <cstdlib>

#include "qloco_nlp_core.hpp"

namespace qloco {

struct TickArgs {
  qloco_nlp_params prm;
  qloco_nlp_tick_params tp;
  int64_t batch;
  const double *nws;
  double *tws;
  const int32_t *t_int, *stop;
  const double *com;
  const int32_t *sched, *sst;
  double *com_traj, *rlfoot;
  int32_t *rs, *status;
};

// both feet's xyz at array index k: not yet written -> the values of
// Initialize (:496-499); no longer held -> NaN
__device__ __forceinline__ void tk_ring_rd(const double *w, int64_t B, int k, int last, double sw0, double (&o)[6]) {
  if (k > last + 1) {
    o[0] = 0.0; o[1] = -sw0; o[2] = 0.0; o[3] = 0.0; o[4] = sw0; o[5] = 0.0;
  } else if (k < 0 || k <= last + 1 - TK_RING) {
#pragma unroll
    for (int c = 0; c < 6; ++c) o[c] = __builtin_nan("");
  } else {
    const int s = k % TK_RING;
#pragma unroll
    for (int c = 0; c < 6; ++c) o[c] = w[(int64_t)(TK_RINGF + s * 6 + c) * B];
  }
}

// 64-bit value of lane `src` of this lane's 8-lane group
__device__ __forceinline__ double tk_shfl8(double v, int src) { return __shfl(v, src, 8); }

// the three needed columns of AAA.inverse(), one robot per lane: r[q][m]
__device__ __forceinline__ void tk_height_cols_lane(const double (&tp3)[3], double (&r)[7][3]) {
  double m[7][7];
  constexpr int kind[7] = {1, 2, 0, 0, 0, 1, 2}, which[7] = {0, 0, 0, 1, 2, 2, 2};
#pragma unroll
  for (int q = 0; q < 7; ++q) {
    const double t = tp3[which[q]];
    double pw[7];
    nlp_powers(t, pw);
    const double t2 = pw[2], t3 = pw[3], t4 = pw[4], t5 = pw[5], t6 = pw[6];
    if (kind[q] == 0) {
      m[q][0] = t6; m[q][1] = t5; m[q][2] = t4; m[q][3] = t3; m[q][4] = t2; m[q][5] = t; m[q][6] = 1.0;
    } else if (kind[q] == 1) {
      m[q][0] = 6 * t5; m[q][1] = 5 * t4; m[q][2] = 4 * t3; m[q][3] = 3 * t2; m[q][4] = 2 * t; m[q][5] = 1.0; m[q][6] = 0.0;
    } else {
      m[q][0] = 30 * t4; m[q][1] = 20 * t3; m[q][2] = 12 * t2; m[q][3] = 6 * t; m[q][4] = 2.0; m[q][5] = 0.0; m[q][6] = 0.0;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) r[q][c] = (q == c + 2) ? 1.0 : 0.0;  // columns 2, 3, 4 of the identity
  }
  nlp_lu<7, 3>(m, r);
  nlp_lu_solve<7, 3>(m, r);
}

// the same three columns, one robot per 8-lane group: lane li < 7 holds row li
// of the matrix and of the right-hand sides (lane 7 idles); the pivot search
// reads column k of every row through cross-lane moves, the swap exchanges
// two lanes' rows, and every row sees the operations of nlp_lu / nlp_lu_solve
// in the same order, so the result is the lane form's, bit for bit.  Every
// lane returns the full r.
__device__ __forceinline__ void tk_height_cols_group(const double (&tp3)[3], int li, double (&r)[7][3]) {
  const int kind = (li == 0 || li == 5) ? 1 : ((li == 1 || li == 6) ? 2 : 0);
  const double t = li < 3 ? tp3[0] : (li == 3 ? tp3[1] : tp3[2]);
  double pw[7];
  nlp_powers(t, pw);
  const double t2 = pw[2], t3 = pw[3], t4 = pw[4], t5 = pw[5], t6 = pw[6];
  double row[7], rr[3];
  row[0] = kind == 0 ? t6 : (kind == 1 ? 6 * t5 : 30 * t4);
  row[1] = kind == 0 ? t5 : (kind == 1 ? 5 * t4 : 20 * t3);
  row[2] = kind == 0 ? t4 : (kind == 1 ? 4 * t3 : 12 * t2);
  row[3] = kind == 0 ? t3 : (kind == 1 ? 3 * t2 : 6 * t);
  row[4] = kind == 0 ? t2 : (kind == 1 ? 2 * t : 2.0);
  row[5] = kind == 0 ? t : (kind == 1 ? 1.0 : 0.0);
  row[6] = kind == 0 ? 1.0 : 0.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) rr[c] = (li == c + 2) ? 1.0 : 0.0;
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    int p = k;
    double best = fabs(tk_shfl8(row[k], k));
#pragma unroll
    for (int q = k + 1; q < 7; ++q) {
      const double v = fabs(tk_shfl8(row[k], q));
      const bool g = v > best;
      p = g ? q : p;
      best = g ? v : best;
    }
    const int src = li == k ? p : (li == p ? k : li);
#pragma unroll
    for (int c = 0; c < 7; ++c) row[c] = tk_shfl8(row[c], src);
#pragma unroll
    for (int c = 0; c < 3; ++c) rr[c] = tk_shfl8(rr[c], src);
    const bool below = li > k;
    const double pk = tk_shfl8(row[k], k);
    const double l = row[k] / pk;
    row[k] = below ? l : row[k];
#pragma unroll
    for (int c = k + 1; c < 7; ++c) {
      const double pc = tk_shfl8(row[c], k);
      const double v = row[c] - l * pc;
      row[c] = below ? v : row[c];
    }
  }
#pragma unroll
  for (int m = 0; m < 3; ++m) {
#pragma unroll
    for (int c = 0; c < 7; ++c) {  // forward: row q takes y[c], c = 0 .. q - 1, in ascending order
      const double yc = tk_shfl8(rr[m], c);
      const double v = rr[m] - row[c] * yc;
      rr[m] = li > c ? v : rr[m];
    }
    double x[7];
#pragma unroll
    for (int q = 6; q >= 0; --q) {  // back: lane q's row, c = q + 1 .. 6 in ascending order
      double acc = rr[m];
#pragma unroll
      for (int c = q + 1; c < 7; ++c) acc = acc - row[c] * x[c];
      x[q] = tk_shfl8(acc / row[q], q);
    }
#pragma unroll
    for (int q = 0; q < 7; ++q) r[q][m] = x[q];
  }
}

// GW = 1: one robot per lane.  GW = 8: one robot per 8-lane group; the 7 x 7
// system is spread over the group, everything else runs on its first lane.
template <int GW>
__global__ __launch_bounds__(64) void nlp_tick_kernel(const TickArgs a) {
  const int64_t rb = (int64_t)blockIdx.x * (64 / GW) + threadIdx.x / GW;
  const int li = threadIdx.x % GW;
  const bool wr = li == 0;  // this lane stores
  if (rb >= a.batch) return;
  const int64_t B = a.batch;
  const double nan = __builtin_nan("");
  const double *const ts = a.nws + rb * NLP_NS;
  const double *const tx = a.nws + B * NLP_NS + rb * NLP_NS;
  const double *const fm = a.nws + 2 * B * NLP_NS + rb;  // section-14 field f at fm[f * B]
  double *const w = a.tws + rb;                          // field f at w[f * B]
  double *const ct = a.com_traj + 38 * rb;
  double *const rl = a.rlfoot + 18 * rb;
  const int sst = a.sst[rb];
  if (sst == QLOCO_NLP_FINISHED || sst == QLOCO_BAD_SIZE) {
    // outside the plan: neither record is touched
    if (!wr) return;
    for (int k = 0; k < 38; ++k) ct[k] = nan;
    for (int k = 0; k < 18; ++k) rl[k] = nan;
    a.rs[rb] = 2;
    if (a.status) a.status[rb] = sst;
    return;
  }
  const double dt = a.prm.dt, hcom = a.tp.hcom;
  const int i = a.t_int[rb];
  const int period = a.sched[4 * rb + 0], bjxx = a.sched[4 * rb + 2], bjx1 = a.sched[4 * rb + 3];
  const double *const com = a.com + 18 * rb;

  // ---- CoM_height_solve (:2361-2473) with the previous tick's _bjx1
  const int b0 = nlp_int(w[(int64_t)TK_BJX1 * B]);
  double cz[3] = {hcom, hcom, hcom}, cvz[3] = {0.0, 0.0, 0.0}, caz[3] = {0.0, 0.0, 0.0};
  if (b0 >= 2) {
    const double tsb = nlp_at(ts, 1, b0 - 1);
    const double tp3[3] = {0.0001, tsb / 2 + 0.0001, tsb + 0.0001};
    double r[7][3];  // columns 2, 3, 4 of AAA.inverse()
    if constexpr (GW == 1)
      tk_height_cols_lane(tp3, r);
    else
      tk_height_cols_group(tp3, li, r);
    const double z0 = nlp_at(w + (int64_t)TK_FZ * B, B, b0 - 2), z1 = nlp_at(w + (int64_t)TK_FZ * B, B, b0 - 1);
    const double p2 = z0 + hcom, p3 = (z0 + z1) / 2 + hcom, p4 = z1 + hcom;
    double co[7];
#pragma unroll
    for (int q = 0; q < 7; ++q) co[q] = ((0.0 + r[q][0] * p2) + r[q][1] * p3) + r[q][2] * p4;
    const double rt0 = round(nlp_at(tx, 1, b0 - 1) / dt);
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      const double t = ((double)(i + s + 1) - rt0) * dt;
      double pw[7];
      nlp_powers(t, pw);
      const double t2 = pw[2], t3 = pw[3], t4 = pw[4], t5 = pw[5], t6 = pw[6];
      cz[s] = (((((t6 * co[0] + t5 * co[1]) + t4 * co[2]) + t3 * co[3]) + t2 * co[4]) + t * co[5]) + 1.0 * co[6];
      cvz[s] = ((((((6 * t5) * co[0] + (5 * t4) * co[1]) + (4 * t3) * co[2]) + (3 * t2) * co[3]) + (2 * t) * co[4]) +
                1.0 * co[5]) + 0.0 * co[6];
      caz[s] = ((((((30 * t4) * co[0] + (20 * t3) * co[1]) + (12 * t2) * co[2]) + (6 * t) * co[3]) + 2.0 * co[4]) +
                0.0 * co[5]) + 0.0 * co[6];
    }
    }
  if (!wr) return;  // the group's other lanes only carry rows of the 7 x 7 system
  w[(int64_t)TK_BJX1 * B] = (double)bjx1;  // :1038

  // ---- _Zsc(i), (i + 1), (i + 2): _footz_ref of the step (k + 1) dt falls in under the initial _tx
  double zs[3];
  {
    const int nsum = (NLP_NS - 1) * nlp_int(round(a.prm.tstep / dt));
    int j0 = 0, j1 = 0, j2 = 0;
    bool g0 = true, g1 = true, g2 = true;
    for (int k = 0; k < NLP_NS; ++k) {
      const double t = w[(int64_t)(TK_TX0 + k) * B];
      g0 = g0 && ((i + 1) * dt >= t);
      g1 = g1 && ((i + 2) * dt >= t);
      g2 = g2 && ((i + 3) * dt >= t);
      j0 += g0 ? 1 : 0;
      j1 += g1 ? 1 : 0;
      j2 += g2 ? 1 : 0;
    }
    const double *const fz = w + (int64_t)TK_FZ * B;
    zs[0] = (i + 0 >= nsum - 1) ? 0.0 : nlp_at(fz, B, j0 - 1);
    zs[1] = (i + 1 >= nsum - 1) ? 0.0 : nlp_at(fz, B, j1 - 1);
    zs[2] = (i + 2 >= nsum - 1) ? 0.0 : nlp_at(fz, B, j2 - 1);
  }
  // ---- :950-954 and the 38-vector :1048-1090
  bool fin = true;
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const double comx = com[6 * s + 0], comy = com[6 * s + 1], comvx = com[6 * s + 2], comvy = com[6 * s + 3];
    const double comax = com[6 * s + 4], comay = com[6 * s + 5];
    const double q = (cz[s] - zs[s]) / (caz[s] + 9.8);  // _ggg (:538)
    const double rq = sqrt(q);
    const double zx = comx - q * comax, zy = comy - q * comay, dx = comx + comvx * rq, dy = comy + comvy * rq;
    ct[9 + 4 * s + 0] = zx;
    ct[9 + 4 * s + 1] = zy;
    ct[9 + 4 * s + 2] = dx;
    ct[9 + 4 * s + 3] = dy;
    fin = fin && isfinite(zx) && isfinite(zy) && isfinite(dx) && isfinite(dy) && isfinite(comx) && isfinite(comy) &&
          isfinite(comvx) && isfinite(comvy) && isfinite(comax) && isfinite(comay) && isfinite(cz[s]) &&
          isfinite(cvz[s]) && isfinite(caz[s]);
  }
  ct[0] = com[0];
  ct[1] = com[1];
  ct[2] = cz[0];
  ct[3] = com[2];
  ct[4] = com[3];
  ct[5] = cvz[0];
  ct[6] = com[4];
  ct[7] = com[5];
  ct[8] = caz[0];
  ct[21] = com[10];
  ct[22] = com[11];
  ct[23] = caz[1];
  ct[24] = com[16];
  ct[25] = com[17];
  ct[26] = caz[2];
  ct[27] = (double)bjxx;
  const double *const fxp = fm + (int64_t)ST_FX * B, *const fyp = fm + (int64_t)ST_FY * B;
  const double *const fzp = w + (int64_t)TK_FZ * B;
  {
    const bool in = bjxx >= 0 && bjxx + 1 < NLP_NS;
    const double v28 = in ? nlp_at(fxp, B, bjxx) : nan, v29 = in ? nlp_at(fxp, B, bjxx + 1) : nan;
    const double v30 = in ? nlp_at(fyp, B, bjxx) : nan, v31 = in ? nlp_at(fyp, B, bjxx + 1) : nan;
    const double v32 = in ? nlp_at(fzp, B, bjxx) : nan, v33 = in ? nlp_at(fzp, B, bjxx + 1) : nan;
    ct[28] = v28;
    ct[29] = v29;
    ct[30] = v30;
    ct[31] = v31;
    ct[32] = v32;
    ct[33] = v33;
    if (in) fin = fin && isfinite(v28) && isfinite(v29) && isfinite(v30) && isfinite(v31) && isfinite(v32) && isfinite(v33);
  }
  {
    const double v35 = nlp_at(ts, 1, period - 1), v36 = nlp_at(fm + (int64_t)ST_LXX * B, B, period - 1);
    const double v37 = nlp_at(fm + (int64_t)ST_LYY * B, B, period - 1);
    ct[34] = (double)(period - 1);
    ct[35] = v35;
    ct[36] = v36;
    ct[37] = v37;
    fin = fin && isfinite(v35) && isfinite(v36) && isfinite(v37);
  }

  // ---- Foot_trajectory_solve_mod2 (:2039-2358)
  const int t_end = nlp_int(w[(int64_t)TK_TEND * B]);
  const double sw0 = w[(int64_t)TK_SW0 * B];
  const int last = nlp_int(w[(int64_t)TK_LAST * B]);
  const bool stop = a.stop ? a.stop[rb] != 0 : false;
  if (stop || i > t_end)  // :2043-2050
    for (int k = (bjx1 + 1 > 0 ? bjx1 + 1 : 0); k < NLP_NS; ++k) w[(int64_t)(TK_LIFT + k) * B] = 0.0;
  double cur[6], nxt[6], vel[6] = {0, 0, 0, 0, 0, 0}, acc[6] = {0, 0, 0, 0, 0, 0};
  int rs = 2;
  if (bjx1 >= 2 && i <= t_end) {  // :2076
    const int b = bjx1;
    const double txb = nlp_at(tx, 1, b - 1), tsb = nlp_at(ts, 1, b - 1), tdb = nlp_at(fm + (int64_t)ST_TD * B, B, b - 1);
    const double rt = round(txb / dt);
    double H[6];
    tk_ring_rd(w, B, (rt == rt) ? nlp_int(rt) - 2 : -1, last, sw0, H);
    const bool swr = (b % 2) == 0;  // the right foot swings (left support)
    rs = swr ? 0 : 1;
    double sg[3], sn[3], sv[3] = {0, 0, 0}, sa[3] = {0, 0, 0};  // swing foot: at j, at j + 1, velocity, acceleration
    const double st0 = swr ? H[3] : H[0], st1 = swr ? H[4] : H[1], st2 = swr ? H[5] : H[2];  // :2082-2088, :2191-2197
    if (((double)(i + 1) - rt) * dt < tdb) {  // :2091, :2200: double support
      rs = 2;
#pragma unroll
      for (int c = 0; c < 3; ++c) sg[c] = sn[c] = swr ? H[c] : H[3 + c];
    } else {
      const double t_des = ((double)(i + 1) - rt + 1) * dt;
      const double f2x = nlp_at(fxp, B, bjxx), f2y = bjxx == 0 ? -sw0 : nlp_at(fyp, B, bjxx), f2z = nlp_at(fzp, B, bjxx);
      if (fabs(t_des - tsb) <= 0.0005) {  // :2113, :2226: landing
        sg[0] = sn[0] = f2x;
        sg[1] = sn[1] = f2y;
        sg[2] = sn[2] = f2z;
      } else {
        const double tpl[3] = {t_des - dt, (tdb + tsb) / 2 + 0.0001, tsb};
        double m[4][4];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const double t = tpl[q], t2 = t * t;
          m[q][0] = t2 * t;
          m[q][1] = t2;
          m[q][2] = t;
          m[q][3] = 1.0;
        }
        m[3][0] = 3 * (tsb * tsb);
        m[3][1] = 2 * tsb;
        m[3][2] = 1.0;
        m[3][3] = 0.0;
        double P[6];
        tk_ring_rd(w, B, i - 1, last, sw0, P);
        const double f0x = nlp_at(fxp, B, bjxx - 2), f0y = bjxx == 2 ? -sw0 : nlp_at(fyp, B, bjxx - 2);
        const double f0z = nlp_at(fzp, B, bjxx - 2);
        double ry = w[(int64_t)TK_RY * B];
        if (((double)(i + 1) - rt) * dt < tdb + dt) {  // :2150, :2268
          ry = (f2y + f0y) / 2;
          w[(int64_t)TK_RY * B] = ry;
        }
        const double zmid = (f0z < f2z ? f2z : f0z) + nlp_at(w + (int64_t)TK_LIFT * B, B, b - 1);
        const double plan[3][3] = {{swr ? P[0] : P[3], (f0x + f2x) / 2, f2x},
                                   {swr ? P[1] : P[4], ry, f2y},
                                   {swr ? P[2] : P[5], zmid, f2z}};
        // the three right-hand sides as columns; one pivoted LU, three substitutions
        double rh[4][3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
          rh[0][ax] = plan[ax][0];
          rh[1][ax] = plan[ax][1];
          rh[2][ax] = plan[ax][2];
          rh[3][ax] = 0.0;
        }
        nlp_lu<4, 3>(m, rh);
        nlp_lu_solve<4, 3>(m, rh);
        const double t = t_des, t2 = t * t, t3 = t2 * t;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
          const double co[4] = {rh[0][ax], rh[1][ax], rh[2][ax], rh[3][ax]};
          const double pos = ((t3 * co[0] + t2 * co[1]) + t * co[2]) + 1.0 * co[3];
          const double v = (((3 * t2) * co[0] + (2 * t) * co[1]) + 1.0 * co[2]) + 0.0 * co[3];
          const double ac = (((6 * t) * co[0] + 2.0 * co[1]) + 0.0 * co[2]) + 0.0 * co[3];
          sg[ax] = pos;
          sv[ax] = v;
          sa[ax] = ac;
          sn[ax] = pos + dt * v;  // :2181-2183
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double stc = c == 0 ? st0 : (c == 1 ? st1 : st2);
      cur[c] = swr ? sg[c] : stc;
      cur[3 + c] = swr ? stc : sg[c];
      nxt[c] = swr ? sn[c] : stc;
      nxt[3 + c] = swr ? stc : sn[c];
      vel[c] = swr ? sv[c] : 0.0;
      vel[3 + c] = swr ? 0.0 : sv[c];
      acc[c] = swr ? sa[c] : 0.0;
      acc[3 + c] = swr ? 0.0 : sa[c];
    }
  } else {
    tk_ring_rd(w, B, i + 1, last, sw0, nxt);
    if (i > t_end) {  // :2314-2322
      tk_ring_rd(w, B, i - 1, last, sw0, cur);
    } else {  // :2325-2326
      tk_ring_rd(w, B, i, last, sw0, cur);
      cur[1] = -sw0;
      cur[4] = sw0;
    }
  }
  {
    const int s0 = i % TK_RING, s1 = (i + 1) % TK_RING;  // i >= 1 here
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      w[(int64_t)(TK_RINGF + s0 * 6 + c) * B] = cur[c];
      w[(int64_t)(TK_RINGF + s1 * 6 + c) * B] = nxt[c];
    }
    w[(int64_t)TK_LAST * B] = (double)i;
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    rl[c] = cur[c];
    rl[6 + c] = vel[c];
    rl[12 + c] = acc[c];
    fin = fin && isfinite(cur[c]) && isfinite(vel[c]) && isfinite(acc[c]);
  }
  a.rs[rb] = rs;
  if (a.status) a.status[rb] = (sst == QLOCO_OK && !fin) ? QLOCO_NAN : sst;
}

// the members of FootStepInputs / Initialize the tick reads beyond section 14's
// record (:67, :71-75, :176-180, :195-206, :488, :496-500, :593)
__global__ __launch_bounds__(256) void nlp_tick_init_kernel(int64_t B, double *ws, double dt, double tstep,
                                                            double lift_height, const double *stepwidth,
                                                            const double *stepheight) {
  const int64_t rb = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (rb >= B) return;
  double *const w = ws + rb;
  const double sw0 = stepwidth[rb] / 2, sh = stepheight ? stepheight[rb] : 0.0;
  double z = 0.0, t = 0.0;
  for (int j = 0; j < NLP_NS; ++j) {
    w[(int64_t)(TK_FZ + j) * B] = z;
    z = z + sh;
    double lh = lift_height;
    if (j >= NLP_NS - 2) lh = 0.0;
    if (j == NLP_NS - 3) lh = lift_height / 2;
    w[(int64_t)(TK_LIFT + j) * B] = lh;
    w[(int64_t)(TK_TX0 + j) * B] = t;
    if (j == NLP_NS - 1) w[(int64_t)TK_TEND * B] = round((t - 2 * tstep) / dt);
    t = t + tstep;
    t = round(t / dt) * dt - 0.000001;
  }
  w[(int64_t)TK_BJX1 * B] = 0.0;
  w[(int64_t)TK_RY * B] = 0.0;
  w[(int64_t)TK_SW0 * B] = sw0;
  w[(int64_t)TK_LAST * B] = 0.0;
  for (int s = 0; s < TK_RING; ++s) {
    w[(int64_t)(TK_RINGF + s * 6 + 0) * B] = 0.0;
    w[(int64_t)(TK_RINGF + s * 6 + 1) * B] = -sw0;
    w[(int64_t)(TK_RINGF + s * 6 + 2) * B] = 0.0;
    w[(int64_t)(TK_RINGF + s * 6 + 3) * B] = 0.0;
    w[(int64_t)(TK_RINGF + s * 6 + 4) * B] = sw0;
    w[(int64_t)(TK_RINGF + s * 6 + 5) * B] = 0.0;
  }
}

}  // namespace qloco

using namespace qloco;

extern "C" void qloco_nlp_tick_params_default(qloco_nlp_tick_params *p) {
  if (!p) return;
  p->lift_height = 0.03;  // NLPRTControlClass.cpp:48
  p->hcom = 0.309458;     // RobotPara_Z_C - _height_offset (NLPClass_sqp.cpp:212, NLPClass.h:37)
  for (int k = 0; k < 6; ++k) p->reserved[k] = 0;
}

// kernel form: 1 (one robot per lane, shipped) or 8 (one robot per 8-lane
// group, the A/B form); QLOCO_NLP_TICK_GW presets it
static std::atomic<int> g_tick_gw{[] {
  const char *e = getenv("QLOCO_NLP_TICK_GW");
  return (e && atoi(e) == 8) ? 8 : 1;
}()};

extern "C" int qloco_nlp_tick_set_group_width(int gw) {
  if (gw != 1 && gw != 8) return QLOCO_ERR_ARG;
  return g_tick_gw.exchange(gw);
}

extern "C" int64_t qloco_nlp_tick_workspace_bytes(int64_t batch) {
  if (batch <= 0 || batch > kNlpMaxBatch) return -1;
  return batch * (int64_t)TK_WS * (int64_t)sizeof(double);
}

extern "C" int qloco_nlp_tick_init(const qloco_nlp_params *prm, const qloco_nlp_tick_params *tick_prm, int64_t batch,
                                   void *nlp_workspace, void *tick_workspace, const double *steplength,
                                   const double *stepwidth, const double *stepheight, void *stream) {
  if (!nlp_tick_params_ok(prm, tick_prm) || batch <= 0 || batch > kNlpMaxBatch || !nlp_workspace || !tick_workspace ||
      !steplength || !stepwidth)
    return QLOCO_ERR_ARG;
  const int r = qloco_nlp_init(prm, batch, nlp_workspace, steplength, stepwidth, stepheight, stream);
  if (r != QLOCO_OK) return r;
  hipLaunchKernelGGL(nlp_tick_init_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     batch, (double *)tick_workspace, prm->dt, prm->tstep, tick_prm->lift_height, stepwidth,
                     stepheight);
  QLOCO_HIP_CHECK(hipGetLastError(), "nlp_tick_init_kernel launch");
  return QLOCO_OK;
}

extern "C" int qloco_nlp_tick(const qloco_nlp_params *prm, const qloco_nlp_tick_params *tick_prm, int64_t batch,
                              void *nlp_workspace, void *tick_workspace, const int32_t *t_int,
                              const double *estimated_state, const double *rfoot_feedback,
                              const double *lfoot_feedback, const int32_t *stop_walking, double *com_traj,
                              double *rlfoot_traj, int32_t *right_support, double *vari_ini, int32_t *sched,
                              double *step, double *com, int32_t *pass_status, int32_t *pass_iters, int32_t *status,
                              void *stream) {
  if (!nlp_tick_params_ok(prm, tick_prm) || batch <= 0 || batch > kNlpMaxBatch || !nlp_workspace || !tick_workspace ||
      !t_int || !estimated_state || !rfoot_feedback || !lfoot_feedback || !com_traj || !rlfoot_traj ||
      !right_support || !vari_ini)
    return QLOCO_ERR_ARG;
  double *const tws = (double *)tick_workspace;
  double *const com_s = com ? com : tws + (int64_t)TK_S_COM * batch;
  int32_t *const sched_s = sched ? sched : (int32_t *)(tws + (int64_t)TK_S_SCHED * batch);
  int32_t *const st_s = (int32_t *)(tws + (int64_t)TK_S_STATUS * batch);
  const int r = qloco_nlp_step_timing(prm, batch, nlp_workspace, t_int, estimated_state, rfoot_feedback,
                                      lfoot_feedback, vari_ini, sched_s, step, com_s, pass_status, pass_iters, st_s,
                                      stream);
  if (r != QLOCO_OK) return r;
  TickArgs a;
  a.prm = *prm;
  a.tp = *tick_prm;
  a.batch = batch;
  a.nws = (const double *)nlp_workspace;
  a.tws = tws;
  a.t_int = t_int;
  a.stop = stop_walking;
  a.com = com_s;
  a.sched = sched_s;
  a.sst = st_s;
  a.com_traj = com_traj;
  a.rlfoot = rlfoot_traj;
  a.rs = right_support;
  a.status = status;
  if (g_tick_gw.load(std::memory_order_relaxed) == 8)
    hipLaunchKernelGGL(nlp_tick_kernel<8>, dim3((unsigned)((batch + 7) / 8)), dim3(64), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(nlp_tick_kernel<1>, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
  QLOCO_HIP_CHECK(hipGetLastError(), "nlp_tick_kernel launch");
  return QLOCO_OK;
}

extern "C" int qloco_nlp_tick_get_state(int64_t batch, const void *tick_workspace, double *state, void *stream) {
  return nlp_record_copy<NlpTickRecord, false>(batch, tick_workspace, state, stream, "nlp_tick_get_kernel launch");
}

extern "C" int qloco_nlp_tick_set_state(int64_t batch, void *tick_workspace, const double *state, void *stream) {
  return nlp_record_copy<NlpTickRecord, true>(batch, tick_workspace, state, stream, "nlp_tick_set_kernel launch");
}

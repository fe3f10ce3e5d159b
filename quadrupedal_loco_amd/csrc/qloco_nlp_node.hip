// qloco_nlp_node.hip -- the slow planner's node tick, batched (fp64, gfx950):
// /rt2nrt/state in, the /MPC/Gait row out.
//
// qloco_nlp_node_tick is three launches on one stream: a pre-kernel (the node
// loop's start latch and counter, gait_nlp_kmp.cpp:106-110, and the branch of
// NLPRTControlClass::WalkingReactStepping, NLPRTControlClass.cpp:191-285),
// qloco_nlp_tick unchanged, and a post-kernel with what rt_nlp_gait (:436-596)
// and WalkingReactStepping do around it: the _nTdx > 3 tail of the ZMP
// roll-out (NLPClass_sqp.cpp:938-951; line numbers without a file are that
// file's), Zmp_distributor / zmp_interpolation / Force_torque_calculate
// (:3650-3895), X_CoM_position_squat (:2958-3015) and the 100-slot row
// (NLPRTControlClass.cpp:288-392).  tests/nlp_node_ref.py is the restatement
// (compile with -ffp-contract=off); operation order is its formulation A's.
//
// One robot per lane.  The row lives in the node record, field-major, and only
// the slots a branch assigns are stored there; the 800-byte row of gait_msg is
// then copied out of the record in one of two forms with identical bits
// (qloco_nlp_node_set_form): each lane writes its own row, or (shipped) the
// wave stages 16 rows at a time through LDS and writes them coalesced.
//
// The 7 x 7 system of CoM_height_solve is solved again for the tail: its
// coefficients are not an output of section 15.  The powers, the LU, the fill
// of AAA (the host's too, for the squat polynomial), the polynomial and the
// three records' layouts are those of qloco_nlp_core.hpp, which the tick
// kernel includes as well; the block that puts them together keeps the order
// this kernel was tuned in (profiles/nlp_core_ab.txt).
#include <atomic>
#include <cmath>
#include <cstdlib>

#include "qloco_nlp_core.hpp"

namespace qloco {

constexpr int ND_TAIL = 9;  // largest _nTdx
constexpr int ND_TILE = 16; // rows per LDS pass

struct NodeArgs {
  qloco_nlp_params prm;
  qloco_nlp_tick_params tp;
  qloco_nlp_node_params np;
  int64_t batch;
  const double *nws, *tws;
  double *ws;
  const double *nrt;
  double *gait;
  int32_t *sched, *status;
  int wmax;                       // _walkdtime_max
  double wsub;                    // (int)_height_offset_time / _dtx
  double ch[ND_TAIL], sh[ND_TAIL]; // cosh / sinh of _Wn _dt jxx, jxx = 1 .. 9
  double sq[7];                   // the squat polynomial's coefficients
};

struct NodeScratch {
  double *ct, *rl, *com, *vari, *est, *rf, *lf, *prev;
  int32_t *t_int, *rs, *sched, *st, *branch;
};

__host__ __device__ __forceinline__ NodeScratch node_scratch(double *ws, int64_t B) {
  double *const s = ws + (int64_t)ND_REC * B;
  NodeScratch o;
  o.ct = s + (int64_t)NS_CT * B;
  o.rl = s + (int64_t)NS_RL * B;
  o.com = s + (int64_t)NS_COM * B;
  o.vari = s + (int64_t)NS_VARI * B;
  o.est = s + (int64_t)NS_EST * B;
  o.rf = s + (int64_t)NS_RF * B;
  o.lf = s + (int64_t)NS_LF * B;
  o.prev = s + (int64_t)NS_PREV * B;
  int32_t *const n = (int32_t *)(s + (int64_t)NS_INT * B);
  o.t_int = n;
  o.rs = n + B;
  o.sched = n + 2 * B;
  o.st = n + 6 * B;
  o.branch = n + 7 * B;
  return o;
}

// _zmpx_real / _zmpy_real at array index k
__device__ __forceinline__ void nd_ring_rd(const double *w, int64_t B, int k, double &x, double &y) {
  if (k < 0) {
    x = y = __builtin_nan("");
    return;
  }
  const int s = k % ND_RING;
  const double tag = w[(int64_t)(ND_RINGF + 3 * s) * B];
  if (tag == (double)k) {
    x = w[(int64_t)(ND_RINGF + 3 * s + 1) * B];
    y = w[(int64_t)(ND_RINGF + 3 * s + 2) * B];
  } else if (tag > (double)k) {  // a later index has taken the entry
    x = y = __builtin_nan("");
  } else {  // never written (:526)
    x = y = 0.0;
  }
}

__device__ __forceinline__ void nd_ring_wr(double *w, int64_t B, int k, double x, double y) {
  const int s = k % ND_RING;  // k >= 1
  w[(int64_t)(ND_RINGF + 3 * s) * B] = (double)k;
  w[(int64_t)(ND_RINGF + 3 * s + 1) * B] = x;
  w[(int64_t)(ND_RINGF + 3 * s + 2) * B] = y;
}

// a diagonal 3 x 3 times a vector as Eigen sums the full row
__device__ __forceinline__ void nd_diag(const double (&c)[3], const double (&v)[3], double (&o)[3]) {
  o[0] = (c[0] * v[0] + 0.0 * v[1]) + 0.0 * v[2];
  o[1] = (0.0 * v[0] + c[1] * v[1]) + 0.0 * v[2];
  o[2] = (0.0 * v[0] + 0.0 * v[1]) + c[2] * v[2];
}

__device__ __forceinline__ void nd_cross(const double (&a)[3], const double (&b)[3], double (&o)[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// ---- stage 1: the node loop's counter and latch, the branch, section 15's inputs
__global__ __launch_bounds__(256) void nlp_node_pre_kernel(const NodeArgs a) {
  const int64_t rb = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t B = a.batch;
  if (rb >= B) return;
  double *const w = a.ws + rb;
  const NodeScratch s = node_scratch(a.ws, B);
  const double *const msg = a.nrt + (int64_t)QLOCO_NRT_MSG_LEN * rb;
  double count = w[(int64_t)ND_COUNT * B];
  bool latch = w[(int64_t)ND_LATCH * B] != 0.0;
  if (msg[0] > 0) {  // gait_nlp_kmp.cpp:106-110
    latch = true;
    count = count + 1;
    w[(int64_t)ND_COUNT * B] = count;
    w[(int64_t)ND_LATCH * B] = 1.0;
  }
  int branch, w1 = 0, ti = 0;
  if (!(w[(int64_t)ND_STOP * B] < 1)) {  // :120
    branch = QLOCO_NLP_NODE_STOPPED;
  } else {
    w1 = nlp_int(count) - nlp_int(w[(int64_t)ND_RESTART * B]);  // NLPRTControlClass.cpp:196
    if (!latch) {
      branch = QLOCO_NLP_NODE_NOT_STARTED;
    } else if (w1 * a.np.dtx <= a.np.height_offset_time) {  // :207
      branch = QLOCO_NLP_NODE_SQUAT;
    } else {
      w1 = nlp_int((double)w1 - a.wsub);  // :246, an int -= double
      if (w1 < a.wmax) {                 // :247; rt_nlp_gait ticks for _t_int >= 1 (:439)
        branch = QLOCO_NLP_NODE_WALKING;
        ti = w1 >= 1 ? w1 : 0;
      } else {
        branch = QLOCO_NLP_NODE_OVER_TIME;
      }
    }
  }
  s.t_int[rb] = ti;
  s.branch[rb] = branch;
#pragma unroll
  for (int k = 0; k < 6; ++k) s.est[6 * rb + k] = 0.0;  // the member _estimated_state (:445)
  s.lf[2 * rb + 0] = msg[19];
  s.lf[2 * rb + 1] = msg[20];
  s.rf[2 * rb + 0] = msg[22];
  s.rf[2 * rb + 1] = msg[23];
  // what the tick overwrites and the tail needs: _bjx1 (:936) and _td(1) (:933)
  s.prev[2 * rb + 0] = a.tws[(int64_t)TK_BJX1 * B + rb];
  s.prev[2 * rb + 1] = a.nws[2 * B * NLP_NS + (int64_t)(ST_TD + 1) * B + rb];
  if (a.sched) {
    a.sched[QLOCO_NLP_NODE_SCHED_LEN * rb + 1] = w1;
    a.sched[QLOCO_NLP_NODE_SCHED_LEN * rb + 5] = nlp_int(count);
  }
}

// ---- stage 3 of one robot: the branch's assignments to the row in the record
__device__ __forceinline__ void nlp_node_robot(const NodeArgs &a, int64_t rb) {
  const int64_t B = a.batch;
  double *const w = a.ws + rb;
  double *const row = w + (int64_t)ND_ROW * B;  // slot k at row[k * B]
  const NodeScratch s = node_scratch(a.ws, B);
  const int branch = s.branch[rb];
  const double hw = a.prm.half_hip_width, mass = a.np.totalmass;
  int status = QLOCO_OK, ti = 0, ntd = 0, kend = -1;
#define ROW(k) row[(int64_t)(k) * B]
  if (branch == QLOCO_NLP_NODE_NOT_STARTED || branch == QLOCO_NLP_NODE_SQUAT) {
    if (branch == QLOCO_NLP_NODE_SQUAT) {  // NLPRTControlClass.cpp:209-242
      const int w1 = nlp_int(w[(int64_t)ND_COUNT * B]) - nlp_int(w[(int64_t)ND_RESTART * B]);
      const double t_des = w1 * a.np.dtx;
      double z = a.prm.z_c - a.np.height_offset, vz = 0.0, az = 0.0;
      if (t_des <= a.np.height_squat_time) nlp_poly(t_des, a.sq, z, vz, az);
      ROW(0) = 0.0;
      ROW(1) = 0.0;
      ROW(2) = z;
      ROW(36) = 0.0;
      ROW(37) = 0.0;
      ROW(38) = vz;
      ROW(39) = 0.0;
      ROW(40) = 0.0;
      ROW(41) = az;
      ROW(6) = 0.0;
      ROW(7) = hw;
      ROW(8) = 0.0;
      ROW(9) = 0.0;
      ROW(10) = -hw;
      ROW(11) = 0.0;
      if (!(isfinite(z) && isfinite(vz) && isfinite(az))) status = QLOCO_NAN;
    }
    // zmp_ref = (LeftFootPosx + RightFootPosx) / 2 (:232, :268)
    const double zx = (ROW(6) + ROW(9)) / 2, zy = (ROW(7) + ROW(10)) / 2, zz = (ROW(8) + ROW(11)) / 2;
    ROW(12) = zx;
    ROW(13) = zy;
    ROW(14) = zz;
    if (branch == QLOCO_NLP_NODE_SQUAT) {
      ROW(34) = zx;
      ROW(35) = zy;
      ROW(42) = zx;
      ROW(43) = zy;
      ROW(44) = zx;
      ROW(45) = zy;
    }
    const double fz = 9.8 / 2 * mass;
#pragma unroll
    for (int k = 15; k < 27; ++k) ROW(k) = (k == 17 || k == 20) ? fz : 0.0;
    ROW(27) = 1.0;
  } else if (branch == QLOCO_NLP_NODE_OVER_TIME) {  // :256-259
    ROW(99) = 2.0;
    ROW(97) = 2.0;
    w[(int64_t)ND_STOP * B] = 2.0;
    w[(int64_t)ND_RESTART * B] = w[(int64_t)ND_COUNT * B];
  } else if (branch == QLOCO_NLP_NODE_WALKING) {
    const int sst = s.st[rb];
    status = sst;
    ti = s.t_int[rb];
    if (sst != QLOCO_NLP_FINISHED && sst != QLOCO_BAD_SIZE) {
      const int i = ti;
      const double dt = a.prm.dt, hcom = a.tp.hcom;
      const double *const ct = s.ct + 38 * rb, *const rl = s.rl + 18 * rb;
      const int period = s.sched[4 * rb + 0], bjx1 = s.sched[4 * rb + 3];
      const int pi = period - 1;
      const double *const ts = a.nws + rb * NLP_NS;
      const double *const tx = a.nws + B * NLP_NS + rb * NLP_NS;
      const double *const fm = a.nws + 2 * B * NLP_NS + rb;
      const double *const tw = a.tws + rb;
      const double *const fz = tw + (int64_t)TK_FZ * B;
      const int b0 = nlp_int(s.prev[2 * rb + 0]);
      {
        const double r = round(s.prev[2 * rb + 1] / dt);  // :933
        ntd = nlp_int(r) + 1;
        ntd = ntd > ND_TAIL ? ND_TAIL : ntd;
      }
      // ---- the roll-out's ZMP (:938-951): jxx <= 3 are the tick's own bits
#pragma unroll
      for (int q = 0; q < 3; ++q) nd_ring_wr(w, B, i + q, ct[9 + 4 * q], ct[10 + 4 * q]);
      if (ntd > 3) {
        const bool poly = b0 >= 2;
        double co[7] = {0, 0, 0, 0, 0, 0, 0}, rt0 = 0.0;
        // CoM_height_solve (:2376-2429) with the previous tick's _bjx1
        if (poly) {
          const double tsb = nlp_at(ts, 1, b0 - 1);
          const double tp3[3] = {0.0001, tsb / 2 + 0.0001, tsb + 0.0001};
          double pw[3][7], m[7][7], r[7][3];
#pragma unroll
          for (int q = 0; q < 3; ++q) nlp_powers(tp3[q], pw[q]);
          nlp_aaa_fill(pw, m, r);
          nlp_lu<7, 3>(m, r);
          nlp_lu_solve<7, 3>(m, r);
          const double z0 = nlp_at(fz, B, b0 - 2), z1 = nlp_at(fz, B, b0 - 1);
          const double p2 = z0 + hcom, p3 = (z0 + z1) / 2 + hcom, p4 = z1 + hcom;
#pragma unroll
          for (int q = 0; q < 7; ++q) co[q] = ((0.0 + r[q][0] * p2) + r[q][1] * p3) + r[q][2] * p4;
          rt0 = round(nlp_at(tx, 1, b0 - 1) / dt);
        }
        int jz[ND_TAIL - 3];  // _Zsc(i + 3 .. i + 8)
        {
          bool g[ND_TAIL - 3];
#pragma unroll
          for (int q = 0; q < ND_TAIL - 3; ++q) {
            jz[q] = 0;
            g[q] = true;
          }
          for (int k = 0; k < NLP_NS; ++k) {
            const double t = tw[(int64_t)(TK_TX0 + k) * B];
#pragma unroll
            for (int q = 0; q < ND_TAIL - 3; ++q) {
              g[q] = g[q] && ((i + 4 + q) * dt >= t);
              jz[q] += g[q] ? 1 : 0;
            }
          }
        }
        const int nsum = (NLP_NS - 1) * nlp_int(round(a.prm.tstep / dt));
        const double Wn = sqrt(a.prm.g / (a.prm.z_c - 0.0));
        const double xi = nlp_at(fm + (int64_t)ST_CXI * B, B, pi), vxi = nlp_at(fm + (int64_t)ST_CVXI * B, B, pi);
        const double yi = nlp_at(fm + (int64_t)ST_CYI * B, B, pi), vyi = nlp_at(fm + (int64_t)ST_CVYI * B, B, pi);
        const double px = nlp_at(fm + (int64_t)ST_FX * B, B, pi), py = nlp_at(fm + (int64_t)ST_FY * B, B, pi);
#pragma unroll
        for (int q = 3; q < ND_TAIL; ++q) {  // jxx = q + 1
          if (q < ntd) {
            const double c = a.ch[q], sn = a.sh[q];
            const double comx = xi * c + vxi * 1 / Wn * sn + px;
            const double comy = yi * c + vyi * 1 / Wn * sn + py;
            const double comax = (Wn * Wn) * xi * c + vxi * Wn * sn;
            const double comay = (Wn * Wn) * yi * c + vyi * Wn * sn;
            double cz = hcom, cvz = 0.0, caz = 0.0;  // Initialize's, where :2459-2467 write three entries only
            if (poly) nlp_poly(((double)(i + q + 1) - rt0) * dt, co, cz, cvz, caz);
            const double zsc = (i + q >= nsum - 1) ? 0.0 : nlp_at(fz, B, jz[q - 3] - 1);
            const double qq = (cz - zsc) / (caz + 9.8);
            nd_ring_wr(w, B, i + q, comx - qq * comax, comy - qq * comay);
          }
        }
      }
      // ---- zmp_interpolation (:3849-3859): t_des = 0 is clamped
      double Zx, Zy;
      {
        double x1, y1, x0, y0;
        nd_ring_rd(w, B, i, x1, y1);
        nd_ring_rd(w, B, i - 1, x0, y0);
        const double t_des = 0.0001;
        Zx = (x1 - x0) / dt * t_des + x0;
        Zy = (y1 - y0) / dt * t_des + y0;
      }
      // ---- Zmp_distributor (:3666-3830)
      double cl[3], cr[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        cl[k] = w[(int64_t)(ND_COL + k) * B];
        cr[k] = w[(int64_t)(ND_COR + k) * B];
      }
      bool interp = false, swing_l = false;  // swing_l: the interpolated matrix is _Co_L
      double ix = 0.0, iy = 0.0, ex = 0.0, ey = 0.0;
      if (bjx1 >= 2) {
        const double txb = nlp_at(tx, 1, bjx1 - 1), tdb = nlp_at(fm + (int64_t)ST_TD * B, B, bjx1 - 1);
        const double rt = round(txb / dt);
        swing_l = (bjx1 % 2) == 0;
        if (((double)(i + 1) - rt) * dt < tdb) {
          const int n0 = nlp_int(rt), n1 = nlp_int(round((txb + tdb) / dt));
          kend = n1 - 1;
          nd_ring_rd(w, B, n0 - 2, ix, iy);
          nd_ring_rd(w, B, kend, ex, ey);
          interp = true;
        } else {
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            cl[k] = swing_l ? 1.0 : 0.0;
            cr[k] = swing_l ? 0.0 : 1.0;
          }
        }
      } else if (bjx1 == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) cl[k] = cr[k] = 0.5;
      } else {  // _footxyz_real, whose (1, 0) is -_stepwidth(0) (:1046)
        ix = nlp_at(fm + (int64_t)ST_FX * B, B, bjx1 - 1);
        iy = bjx1 == 1 ? -tw[(int64_t)TK_SW0 * B] : nlp_at(fm + (int64_t)ST_FY * B, B, bjx1 - 1);
        ex = nlp_at(fm + (int64_t)ST_FX * B, B, bjx1);
        ey = nlp_at(fm + (int64_t)ST_FY * B, B, bjx1);
        interp = true;
      }
      if (interp) {
        const double dy = ey - iy, dx = ex - ix;
        double c0 = fabs((dy * (Zy - iy) + dx * (Zx - ix)) / (dy * dy + dx * dx));
        double c1 = c0;
        if (c0 > 1) c0 = 1;
        if (c1 > 1) c1 = 1;
        const double c2 = sqrt((c0 * c0 + c0 * c0) / 2);
        const double cc[3] = {c0, c1, c2};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          cl[k] = swing_l ? cc[k] : 1.0 - cc[k];
          cr[k] = swing_l ? 1.0 - cc[k] : cc[k];
        }
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        w[(int64_t)(ND_COL + k) * B] = cl[k];
        w[(int64_t)(ND_COR + k) * B] = cr[k];
      }
      // ---- Force_torque_calculate (:3872-3895): _thetaaxyx, _Lfootxyzx, _Rfootxyzx are zero
      double FL[3], FR[3], ML[3], MR[3];
      {
        const double com[3] = {ct[0], ct[1], ct[2]};
        const double Ft[3] = {mass * (ct[6] - 0.0), mass * (ct[7] - 0.0), mass * (ct[8] - (-9.8))};
        const double jin = mass * (a.np.rad * a.np.rad);
        const double Lt[3] = {jin * 0.0, jin * 0.0, jin * 0.0};
        nd_diag(cr, Ft, FR);
        nd_diag(cl, Ft, FL);
        const double dR[3] = {0.0 - com[0], 0.0 - com[1], 0.0 - com[2]};
        double xr[3], xl[3], Mt[3];
        nd_cross(FR, dR, xr);
        nd_cross(FL, dR, xl);
#pragma unroll
        for (int k = 0; k < 3; ++k) Mt[k] = (Lt[k] - xr[k]) - xl[k];
        nd_diag(cr, Mt, MR);
        nd_diag(cl, Mt, ML);
      }
      // ---- the members rt_nlp_gait assigns (NLPRTControlClass.cpp:445-461, :544-563)
      bool fin = true;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        ROW(k) = ct[k];
        ROW(36 + k) = ct[3 + k];
        ROW(39 + k) = ct[6 + k];
        ROW(9 + k) = rl[k];
        ROW(6 + k) = rl[3 + k];
        ROW(15 + k) = FL[k];
        ROW(18 + k) = FR[k];
        ROW(21 + k) = ML[k];
        ROW(24 + k) = MR[k];
        fin = fin && isfinite(FL[k]) && isfinite(FR[k]) && isfinite(ML[k]) && isfinite(MR[k]);
      }
      ROW(12) = ct[9];
      ROW(13) = ct[10];
      ROW(14) = 0.0;  // _ZMPxy_realx(2)
      ROW(27) = (double)bjx1;
      ROW(34) = ct[11];
      ROW(35) = ct[12];
#pragma unroll
      for (int k = 0; k < 4; ++k) ROW(42 + k) = ct[13 + k];
#pragma unroll
      for (int k = 0; k < 12; ++k) ROW(46 + k) = rl[6 + k];
#pragma unroll
      for (int k = 0; k < 21; ++k) ROW(76 + k) = ct[17 + k];
      ROW(99) = (double)s.rs[rb];
      if (sst == QLOCO_OK && !fin) status = QLOCO_NAN;
    }
  }
  ROW(98) = 0.0;
  if (a.status) a.status[rb] = status;
  if (a.sched) {
    int32_t *const o = a.sched + QLOCO_NLP_NODE_SCHED_LEN * rb;
    o[0] = branch;
    o[2] = ti;
    o[3] = nlp_int(ROW(27));
    o[4] = status;
    o[6] = ntd;
    o[7] = kend;
  }
#undef ROW
}

// FORM 0: the lane writes its robot's row.  FORM 1: 16 rows at a time through
// LDS; the wave then writes 1600 consecutive doubles.
template <int FORM>
__global__ __launch_bounds__(64) void nlp_node_post_kernel(const NodeArgs a) {
  const int64_t B = a.batch;
  const int64_t base = (int64_t)blockIdx.x * 64;
  const int64_t rb = base + threadIdx.x;
  if (rb < B) nlp_node_robot(a, rb);
  const double *const rows = a.ws + (int64_t)ND_ROW * B;
  if constexpr (FORM == 0) {
    if (rb >= B) return;
    for (int k = 0; k < ND_ROWLEN; ++k) a.gait[ND_ROWLEN * rb + k] = rows[(int64_t)k * B + rb];
  } else {
    __shared__ double tile[ND_TILE * ND_ROWLEN];
    const int lane = threadIdx.x, r = lane % ND_TILE, k0 = lane / ND_TILE;
    for (int pass = 0; pass < 64 / ND_TILE; ++pass) {
      const int64_t b0 = base + pass * ND_TILE;
      __syncthreads();  // the record's rows are written; the tile is free
      if (b0 + r < B)
        for (int k = k0; k < ND_ROWLEN; k += 64 / ND_TILE) tile[r * ND_ROWLEN + k] = rows[(int64_t)k * B + b0 + r];
      __syncthreads();
      const int64_t left = B - b0;
      const int n = (left < ND_TILE ? (left < 0 ? 0 : (int)left) : ND_TILE) * ND_ROWLEN;
      for (int e = lane; e < n; e += 64) a.gait[ND_ROWLEN * b0 + e] = tile[e];
    }
  }
}

// NLPRTControlClass() (:86-185)
__global__ __launch_bounds__(256) void nlp_node_init_kernel(int64_t B, double *ws, double z_c, double hw) {
  const int64_t rb = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (rb >= B) return;
  double *const w = ws + rb;
  for (int f = 0; f < ND_REC; ++f) w[(int64_t)f * B] = 0.0;
  for (int s = 0; s < ND_RING; ++s) w[(int64_t)(ND_RINGF + 3 * s) * B] = -1.0;
  w[(int64_t)(ND_ROW + 2) * B] = z_c;   // PelvisPos(2)
  w[(int64_t)(ND_ROW + 7) * B] = hw;    // LeftFootPosx(1)
  w[(int64_t)(ND_ROW + 10) * B] = -hw;  // RightFootPosx(1)
  w[(int64_t)(ND_ROW + 99) * B] = 2.0;  // right_support
}

}  // namespace qloco

using namespace qloco;

extern "C" void qloco_nlp_node_params_default(qloco_nlp_node_params *p) {
  if (!p) return;
  p->dtx = 0.025;               // dt_nlp
  p->height_offset_time = 1;    // NLPRTControlClass.h:18
  p->height_squat_time = 1;     // NLPClass.h:38
  p->height_offset = 0;         // NLPClass.h:37
  p->height_offsetx = 0;        // NLPRTControlClass.h:17
  p->totalmass = 12;            // NLPRTControlClass.cpp:34
  p->rad = 0.2;                 // NLPClass_sqp.cpp:275
  for (int k = 0; k < 9; ++k) p->reserved[k] = 0;
}

// row-store form: 1 (LDS tiles, shipped: the faster of the two in
// profiles/bench_nlp_node.json) or 0 (lane, the A/B form); QLOCO_NLP_NODE_FORM
// presets it
static std::atomic<int> g_node_form{[] {
  const char *e = getenv("QLOCO_NLP_NODE_FORM");
  return (e && e[0] == '0' && e[1] == 0) ? 0 : 1;
}()};

extern "C" int qloco_nlp_node_set_form(int form) {
  if (form != 0 && form != 1) return QLOCO_ERR_ARG;
  return g_node_form.exchange(form);
}

static bool node_params_ok(const qloco_nlp_params *p, const qloco_nlp_tick_params *tp,
                           const qloco_nlp_node_params *np) {
  // The tick's checks first.  Its ring bound, round(t_max / dt) + 4 <= 48, rejects nothing the ND_TAIL bound
  // below accepts (that one needs t_max / dt < 42.5).  Its hcom > 0 was not restated here before: both entry
  // points returned QLOCO_ERR_ARG for it all the same, from the inner qloco_nlp_tick_init / qloco_nlp_tick.
  if (!nlp_tick_params_ok(p, tp) || !np || !(p->t_max > 0)) return false;
  if (!(np->dtx == p->dt) || !(np->height_offset_time >= 0) || !(np->height_offset_time < 1.0e6) ||
      !(np->height_squat_time > 0) || !std::isfinite(np->height_offset) || !(np->totalmass > 0) ||
      !std::isfinite(np->rad))
    return false;
  // _nTdx = round(_td(1) / _dt) + 1 with _td = 0.2 _ts <= 0.2 t_max
  return std::round(0.2 * p->t_max / p->dt) + 1 <= ND_TAIL;
}

extern "C" int64_t qloco_nlp_node_workspace_bytes(int64_t batch) {
  if (batch <= 0 || batch > kNlpMaxBatch) return -1;
  return batch * (int64_t)(ND_REC + ND_SCR) * (int64_t)sizeof(double);
}

extern "C" int qloco_nlp_node_init(const qloco_nlp_params *prm, const qloco_nlp_tick_params *tick_prm,
                                   const qloco_nlp_node_params *node_prm, int64_t batch, void *nlp_workspace,
                                   void *tick_workspace, void *node_workspace, const double *steplength,
                                   const double *stepwidth, const double *stepheight, void *stream) {
  if (!node_params_ok(prm, tick_prm, node_prm) || batch <= 0 || batch > kNlpMaxBatch || !node_workspace)
    return QLOCO_ERR_ARG;
  const int r = qloco_nlp_tick_init(prm, tick_prm, batch, nlp_workspace, tick_workspace, steplength, stepwidth,
                                    stepheight, stream);
  if (r != QLOCO_OK) return r;
  hipLaunchKernelGGL(nlp_node_init_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     batch, (double *)node_workspace, prm->z_c, prm->half_hip_width);
  QLOCO_HIP_CHECK(hipGetLastError(), "nlp_node_init_kernel launch");
  return QLOCO_OK;
}

// com_co = AAA_inv * com_squat_plan of X_CoM_position_squat (:2965-3002): the
// plan times are constants, so the system is solved here, once per call, with
// the LU inverse's three live columns and then the product
static void node_squat_coefficients(const qloco_nlp_params *prm, const qloco_nlp_node_params *np, double (&co)[7]) {
  const double T = np->height_squat_time;
  const double tp3[3] = {0.00001, T / 2 + 0.0001, T + 0.0001};
  double pw[3][7], m[7][7], r[7][3];
  for (int q = 0; q < 3; ++q) {
    pw[q][0] = 1.0;
    for (int n = 1; n <= 6; ++n) pw[q][n] = std::pow(tp3[q], n);
  }
  nlp_aaa_fill(pw, m, r);
  nlp_lu<7, 3>(m, r);
  nlp_lu_solve<7, 3>(m, r);
  const double p2 = prm->z_c, p3 = prm->z_c - np->height_offset / 2, p4 = prm->z_c - np->height_offset;
  for (int q = 0; q < 7; ++q) co[q] = ((0.0 + r[q][0] * p2) + r[q][1] * p3) + r[q][2] * p4;
}

extern "C" int qloco_nlp_node_tick(const qloco_nlp_params *prm, const qloco_nlp_tick_params *tick_prm,
                                   const qloco_nlp_node_params *node_prm, int64_t batch, void *nlp_workspace,
                                   void *tick_workspace, void *node_workspace, const double *nrt_msg,
                                   double *gait_msg, int32_t *sched, int32_t *status, void *stream) {
  if (!node_params_ok(prm, tick_prm, node_prm) || batch <= 0 || batch > kNlpMaxBatch || !nlp_workspace ||
      !tick_workspace || !node_workspace || !nrt_msg || !gait_msg)
    return QLOCO_ERR_ARG;
  NodeArgs a;
  a.prm = *prm;
  a.tp = *tick_prm;
  a.np = *node_prm;
  a.batch = batch;
  a.nws = (const double *)nlp_workspace;
  a.tws = (const double *)tick_workspace;
  a.ws = (double *)node_workspace;
  a.nrt = nrt_msg;
  a.gait = gait_msg;
  a.sched = sched;
  a.status = status;
  {
    // Get_maximal_number(_dtx) + 1 (:3026-3031, NLPRTControlClass.cpp:96)
    const int nT = (int)std::round(prm->tstep / prm->dt);
    const int nsum = (NLP_NS - 1) * nT, omit = 2 * (int)std::round(prm->tstep / prm->dt);
    a.wmax = (int)((nsum - omit - 1) * std::floor(prm->dt / node_prm->dtx)) + 1;
    a.wsub = (int)node_prm->height_offset_time / node_prm->dtx;
    const double Wn = std::sqrt(prm->g / (prm->z_c - 0.0));
    for (int j = 1; j <= ND_TAIL; ++j) {
      const double wn = Wn * prm->dt * j;
      a.ch[j - 1] = std::cosh(wn);
      a.sh[j - 1] = std::sinh(wn);
    }
    node_squat_coefficients(prm, node_prm, a.sq);
  }
  hipLaunchKernelGGL(nlp_node_pre_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     a);
  QLOCO_HIP_CHECK(hipGetLastError(), "nlp_node_pre_kernel launch");
  const NodeScratch s = node_scratch(a.ws, batch);
  const int r = qloco_nlp_tick(prm, tick_prm, batch, nlp_workspace, tick_workspace, s.t_int, s.est, s.rf, s.lf,
                               nullptr, s.ct, s.rl, s.rs, s.vari, s.sched, nullptr, s.com, nullptr, nullptr, s.st,
                               stream);
  if (r != QLOCO_OK) return r;
  const dim3 grid((unsigned)((batch + 63) / 64));
  if (g_node_form.load(std::memory_order_relaxed) == 1)
    hipLaunchKernelGGL(nlp_node_post_kernel<1>, grid, dim3(64), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(nlp_node_post_kernel<0>, grid, dim3(64), 0, (hipStream_t)stream, a);
  QLOCO_HIP_CHECK(hipGetLastError(), "nlp_node_post_kernel launch");
  return QLOCO_OK;
}

extern "C" int qloco_nlp_node_get_state(int64_t batch, const void *node_workspace, double *state, void *stream) {
  return nlp_record_copy<NlpNodeRecord, false>(batch, node_workspace, state, stream, "nlp_node_get_kernel launch");
}

extern "C" int qloco_nlp_node_set_state(int64_t batch, void *node_workspace, const double *state, void *stream) {
  return nlp_record_copy<NlpNodeRecord, true>(batch, node_workspace, state, stream, "nlp_node_set_kernel launch");
}

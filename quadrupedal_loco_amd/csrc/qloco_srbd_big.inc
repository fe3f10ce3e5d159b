// qloco_srbd_big.inc -- the wide SRBD path: instances with 43..80 stance
// (step, leg) pairs (129..240 stance variables, up to N = 20 all-stance).
// Included by qloco_srbd.hip after its helpers (SrbdArgs, k0k2, the block
// reductions, limit_scaling).
//
// Same problem and the same OSQP algorithm as srbd_admm_kernel<W> (ConvexMpc
// build in closed form, swing legs eliminated, Ruiz scaling, rho vector,
// relaxation, termination / adaptive-rho cadence, outputs; DESIGN.md §3), laid
// out for 256 rows: one instance per 512-thread workgroup (8 waves, 2 per
// SIMD).  Thread t owns stance variable r = t & 255 and the column half
// h = t >> 8 of its K^-1 row: columns [HC h, HC h + HC), HC fp32 VGPRs.  The
// kernel is instantiated per half width HC = 96 / 112 / 120 (up to 192 /
// 224 / 240 variables: 64 / 74 / 80 stance legs), so a batch's K rows carry
// no columns beyond its largest instance (DESIGN.md §3g).  A K^-1 matvec is two
// half-row partial sums combined through LDS; the right-hand side is read by
// same-address ds_read_b128 (an LDS broadcast).  Every thread keeps the five
// constraint rows of its leg (leg-replicated: the x, y and z variables of a
// leg and both column halves compute the same row updates), so the leg-local
// couplings of A need no exchange -- two barriers per ADMM iteration.
// The Gauss-Jordan inverse pivots in the order (k mod HC, k div HC) so the
// pivot column always sits in a static register (any pivot order inverts an
// SPD matrix; the +/- symmetry of GJ gives the pivot row from the column).
namespace qloco {

constexpr int kBigVars = 256;  // rows (variables, padded)
constexpr int kBigHalf = 128;  // K^-1 columns per thread, at most
// wide-kernel half widths and the stance legs each admits (2 HC / 3)
constexpr int kBigHC[3] = {96, 112, 120};
__host__ __device__ constexpr int big_bucket_legs(int hc) { return 2 * hc / 3; }
constexpr int kBigThreads = 512;
constexpr int kBigLegs = 4 * kMaxN;

struct BigLds {
  f4v bv[kBigVars][2];       // per var: {b0,b1,b2,e0}, {e1,e2,step,comp}
  float rhs[kBigVars];       // KKT right-hand side (broadcast source)
  float part[2][kBigVars];   // K^-1 rhs partial sums per column half
  float bc[2][kBigVars];     // Gauss-Jordan pivot row (double-buffered)
  float colv[2][kBigVars];   // Gauss-Jordan pivot column
  float xs[kBigVars];        // unscaled x (P x, outputs)
  float ex[kBigVars];        // leg exchange (Ruiz D factors, scaled x)
  float Dc[kBigVars];        // Ruiz column scaling D
  float pm[2][kBigVars];     // Ruiz row-norm partials per column half
  float err[12 * kMaxN];
  float Wc[12 * kMaxN];
  float q2[16];
  float r2[12];
  float x0[16];
  f2v k0k2[kMaxN * (kMaxN + 1)];
  int cst[kBigVars];
  float red[8][16];
  int legtab[kBigLegs];
  int stepstart[kMaxN + 1];
  int nlegs;
  uint8_t ct[kBigLegs];
};

// (Bqp' w)_v from S.Wc (see bqp_t)
__device__ __forceinline__ float big_bqp_t(const BigLds &S, int step, int comp, f4v lo, f4v hi,
                                           float dtm, float dt2m) {
  const float *w = S.Wc + 12 * step;
  float acc = lo.x * w[6] + lo.y * w[7] + lo.z * w[8];
  acc += lo.w * w[0] + hi.x * w[1] + hi.y * w[2];
  acc += dtm * w[9 + comp] + dt2m * w[3 + comp];
  return acc;
}

// Suffix scans of S.err into S.Wc (row_scans with forward = false)
__device__ __forceinline__ void big_suffix(BigLds &S, int N) {
  const int r = threadIdx.x;
  if (r >= 12) return;
  const bool brow = r >= 6;
  float s0 = 0.0f, s1 = 0.0f;
  for (int j = N - 1; j >= 0; --j) {
    s1 += s0;
    s0 += S.err[12 * j + r];
    S.Wc[12 * j + r] = brow ? s0 : s1;
  }
}

// Unscaled (P x)_v (p_times_x): S.xs holds the unscaled x, synced by the caller.
__device__ __forceinline__ float big_p_times_x(BigLds &S, int N, bool valid, int step, int comp,
                                               f4v lo, f4v hi, float r2v, float xu, float dtm,
                                               float dt2m) {
  const int t = threadIdx.x;
  for (int idx = t; idx < 12 * N; idx += kBigThreads) {
    const int j = idx / 12, s = idx - 12 * j;
    const int sg = s / 3, sc = s - 3 * sg;
    const int off = (sg == 0 ? 3 : 0) + sc;
    const float dsc = sg == 1 ? dt2m : dtm;
    const int p0 = S.stepstart[j], p1 = S.stepstart[j + 1];
    float acc = 0.0f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int p = p0 + q;
      const bool ok = p < p1;
      const int vb = 3 * (ok ? p : 0);
      const float *bf = reinterpret_cast<const float *>(&S.bv[vb][0]);
      const float xa = S.xs[vb], xb = S.xs[vb + 1], xc = S.xs[vb + 2];
      const float ev = bf[off] * xa + bf[8 + off] * xb + bf[16 + off] * xc;
      const float xsel = sc == 0 ? xa : (sc == 1 ? xb : xc);
      const float term = (sg & 1) ? dsc * xsel : ev;
      acc += ok ? term : 0.0f;
    }
    S.err[idx] = acc;
  }
  __syncthreads();
  for (int idx = t; idx < 12 * N; idx += kBigThreads) {
    const int j = idx / 12, rr = idx - 12 * j;
    const f2v *kr = &S.k0k2[j * (kMaxN + 1)];
    float acc = 0.0f;
    for (int k = 0; k < N; ++k) acc = fmaf(rr >= 6 ? kr[k].x : kr[k].y, S.err[12 * k + rr], acc);
    S.Wc[idx] = S.q2[rr] * acc;
  }
  __syncthreads();
  return valid ? big_bqp_t(S, step, comp, lo, hi, dtm, dt2m) + r2v * xu : 0.0f;
}

// This thread's half of the closed-form P row (gen_p_row); padding rows are
// identity rows.
template <int HC>
__device__ __forceinline__ void big_p_row(const BigLds &S, f4v lo, f4v hi, int r, int h,
                                          bool valid, int step, int comp, float r2v, float dtm,
                                          float dt2m, float (&K)[HC]) {
  const float bq0 = S.q2[6] * lo.x, bq1 = S.q2[7] * lo.y, bq2 = S.q2[8] * lo.z;
  const float eq0 = S.q2[0] * lo.w, eq1 = S.q2[1] * hi.x, eq2 = S.q2[2] * hi.y;
  const float linb = valid ? S.q2[9 + comp] * dtm * dtm : 0.0f;
  const float line = valid ? S.q2[3 + comp] * dt2m * dt2m : 0.0f;
  const float dadd = valid ? r2v : 1.0f;
  const float cf = (float)comp;
  int kb = step * (kMaxN + 1), rl = r - HC * h;
  asm volatile("" : "+v"(kb), "+v"(rl));
  const f4v *bvh = &S.bv[HC * h][0];
  const int *csth = &S.cst[HC * h];
#pragma unroll
  for (int c = 0; c < HC; ++c) {
    const f4v clo = bvh[2 * c], chi = bvh[2 * c + 1];
    const f2v kk = S.k0k2[kb + csth[c]];
    const bool same = chi.w == cf;
    const float beta = fmaf(bq2, clo.z, fmaf(bq1, clo.y, fmaf(bq0, clo.x, same ? linb : 0.0f)));
    const float epsv = fmaf(eq2, chi.y, fmaf(eq1, chi.x, fmaf(eq0, clo.w, same ? line : 0.0f)));
    float pv = fmaf(kk.y, epsv, kk.x * beta);
    pv += (c == rl) ? dadd : 0.0f;
    K[c] = pv;
  }
}

// The leg's five constraint rows (ConvexMpc.cpp:47-59, :227-249), held by
// every thread of the leg: row i couples its own variable (x for rows 0, 1;
// y for 2, 3; z for 4) with coefficient ao[i] and the z variable with az[i].
struct LegRows {
  float ao[5], az[4];
  float lo[5], up[5];
  float E[5];
  float z[5], y[5];
};

template <bool WS, int HC>
__global__ __launch_bounds__(kBigThreads) __attribute__((amdgpu_waves_per_eu(2)))
void srbd_admm_big_kernel(const SrbdArgs a) {
  __shared__ __attribute__((aligned(16))) BigLds S;
  const int t = threadIdx.x;
  const int wave = t >> 6, lane = t & 63;
  const int h = t >> 8, r = t & (kBigVars - 1);
  const int64_t pos = blockIdx.x;
  if (pos >= (a.count ? (int64_t)*a.count : a.batch)) return;
  const int64_t b = a.list ? (int64_t)a.list[pos] : pos;
  const int N = a.N;
  const float Nf = (float)N;
  const float dt = a.dt;
  const SrbdBody body = srbd_body(a, b);
  const float dtm = dt / body.mass, dt2m = dt * dt / body.mass;

  // ---------------- 1. inputs -> LDS, 2. stance enumeration (srbd_solve_one)
  srbd_load_inputs<kBigThreads>(a, S, b, t);
  __syncthreads();
  srbd_enumerate_stance(a, S, t);
  __syncthreads();
  const int nlegs = uni(S.nlegs);
  const int n = 3 * nlegs;
  if (nlegs < a.leg_lo || nlegs > a.leg_hi) return;  // another launch's instance
  if (nlegs > big_bucket_legs(HC)) {  // uniform
    srbd_refuse<kBigThreads>(a, b, t, QLOCO_BAD_SIZE);
    return;
  }
  if (a.model && srbd_body_bad(body)) {  // uniform; only a row can be
    srbd_refuse<kBigThreads>(a, b, t, QLOCO_ERR_ARG);
    return;
  }
  const int NP = 100 * N;
  bool p_init, p_same;
  float *prec = srbd_persist_record<kBigThreads, WS>(a, S, b, t, p_init, p_same);

  // variable r = 3 * (stance pair pl) + comp; r < n <=> pl < nlegs
  const int pl = r / 3;
  const int comp = r - 3 * pl;
  const bool valid = r < n;
  int step = 0, leg = 0;
  if (valid) {
    const int pr = S.legtab[pl];
    step = pr >> 2;
    leg = pr & 3;
  }
  if (h == 0) S.cst[r] = valid ? step : kMaxN;
  for (int idx = t; idx < N * (kMaxN + 1); idx += kBigThreads) {
    const int sr = idx / (kMaxN + 1), sc = idx - (kMaxN + 1) * sr;
    float K0 = 0.0f, K2 = 0.0f;
    if (sc < N) k0k2((float)sr, (float)sc, Nf, K0, K2);
    S.k0k2[idx] = (f2v){K0, K2};
  }

  // ---------------- 3. SRBD model terms (ConvexMpc.cpp:111-160, compute_grf :502-549)
  const float yaw = S.x0[2];
  const float cy = cosf(yaw), sy = sinf(yaw);
  const float R00 = cy, R01 = sy, R10 = -sy, R11 = cy;  // A1RobotControl.cpp:506-508
  f4v lo, hi;
  {
    float Ii[3][3], ba[3];
    srbd_inertia_inv(cy, sy, body.inertia, Ii);
    srbd_bd_column(Ii, srbd_foot(a.feet, b, N, a.feet_per_step, step, leg), comp, dt, R00, R01,
                   R10, R11, step, valid, ba, lo, hi);
    if (h == 0) {
      S.bv[r][0] = lo;
      S.bv[r][1] = hi;
    }
  }
  const float r2v = valid ? S.r2[3 * leg + comp] : 0.0f;

  // ---------------- 4. gradient g = Bqp' Q (Aqp x0 - x_ref) (ConvexMpc.cpp:219-221)
  for (int idx = t; idx < 12 * N; idx += kBigThreads) {
    const int i = idx / 12, s = idx - 12 * i;
    const float xf = srbd_free_state<12>(S.x0, s, i, dt, R00, R01, R10, R11);
    S.err[idx] = S.q2[s] * (xf - a.xref[b * 13 * N + 13 * i + s]);
  }
  __syncthreads();
  big_suffix(S, N);
  __syncthreads();
  float qv = valid ? big_bqp_t(S, step, comp, lo, hi, dtm, dt2m) : 0.0f;
  const float q_raw = qv;
  float qsv = qv;  // q in the cost scale's ||q|| (persistent resume: the previous call's)
  const int vidx = 12 * step + 3 * leg + comp;  // this variable's slot in u / the record
  const int rowbase = 20 * step + 5 * leg;      // the leg's first constraint row
  if (p_same) qsv = valid ? prec[84 * N + vidx] : 0.0f;

  // ---------------- 5. the leg's constraint rows (unscaled)
  LegRows L;
  {
    const float on = valid ? 1.0f : 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // [1,0,mu] >= 0, [1,0,-mu] <= 0, [0,1,mu] >= 0, [0,1,-mu] <= 0
      L.ao[i] = on;
      L.az[i] = valid ? ((i & 1) ? -body.mu : body.mu) : 0.0f;
      L.lo[i] = valid ? ((i & 1) ? -INFINITY : 0.0f) : 0.0f;
      L.up[i] = valid ? ((i & 1) ? 0.0f : INFINITY) : 0.0f;
    }
    L.ao[4] = on;  // fz in [fz_min * c, fz_max * c]: c = 0 on the literal QP's swing pairs
    const float cflag = valid ? (float)S.ct[4 * step + leg] : 0.0f;
    L.lo[4] = valid ? body.fz_min * cflag : 0.0f;
    L.up[4] = valid ? body.fz_max * cflag : 0.0f;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      L.E[i] = 1.0f;
      L.z[i] = 0.0f;
      L.y[i] = 0.0f;
    }
  }

  float K[HC];
  big_p_row<HC>(S, lo, hi, r, h, valid, step, comp, r2v, dtm, dt2m, K);

  // ---------------- 6. modified Ruiz equilibration (OSQP scaling.c); K keeps
  // the unscaled P until the K assembly
  float Dr = 1.0f, cs = 1.0f;
  {
    float cnP;
    {
      float m = 0.0f;
#pragma unroll
      for (int c = 0; c < HC; ++c) m = fmaxf(m, fabsf(K[c]));
      S.pm[h][r] = m;
      __syncthreads();
      cnP = fmaxf(S.pm[0][r], S.pm[1][r]);
    }
    const float inv_n = 1.0f / (float)(n > 0 ? n : 1);
    for (int it = 0; it < a.scaling; ++it) {
      // column norm of A for this variable (all its rows are its leg's)
      float cnA;
      if (comp == 0) {
        cnA = fmaxf(fabsf(L.ao[0]), fabsf(L.ao[1]));
      } else if (comp == 1) {
        cnA = fmaxf(fabsf(L.ao[2]), fabsf(L.ao[3]));
      } else {
        cnA = fmaxf(fmaxf(fabsf(L.az[0]), fabsf(L.az[1])), fmaxf(fabsf(L.az[2]), fabsf(L.az[3])));
        cnA = fmaxf(cnA, fabsf(L.ao[4]));
      }
      // v_rsq_f32 / v_rcp_f32 (1 ulp): the Ruiz factors are heuristics
      const float Dt = valid ? __builtin_amdgcn_rsqf(limit_scaling(fmaxf(cnP, cnA))) : 1.0f;
      __syncthreads();  // the previous pass's readers of ex / Dc / pm are done
      if (h == 0) {
        S.ex[r] = Dt;
        S.Dc[r] = Dr * Dt;
      }
      __syncthreads();
      const float Dx = valid ? S.ex[3 * pl] : 1.0f, Dy = valid ? S.ex[3 * pl + 1] : 1.0f,
                  Dz = valid ? S.ex[3 * pl + 2] : 1.0f;
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        const float Et = valid ? __builtin_amdgcn_rsqf(limit_scaling(
                                     fmaxf(fabsf(L.ao[i]), i < 4 ? fabsf(L.az[i]) : 0.0f)))
                               : 1.0f;
        const float Down = i < 2 ? Dx : (i < 4 ? Dy : Dz);
        L.ao[i] *= Et * Down;
        if (i < 4) L.az[i] *= Et * Dz;
        L.E[i] *= Et;
      }
      qv *= Dt;
      qsv *= Dt;
      Dr *= Dt;
      // row norm of D P D after this pass (without the running cost scale)
      float m = 0.0f;
      const float *dh = &S.Dc[HC * h];
#pragma unroll
      for (int c = 0; c < HC; ++c) m = fmaxf(m, fabsf(K[c]) * dh[c]);
      S.pm[h][r] = m;
      __syncthreads();
      const float cn2 = Dr * fmaxf(S.pm[0][r], S.pm[1][r]);
      // cost scaling: mean column norm of P vs ||q||_inf
      const float sumP = bsum<8>((valid && h == 0) ? cn2 : 0.0f, S.red);
      float qm[1] = {valid ? fabsf(qsv) : 0.0f};
      bmax<8, 1>(qm, S.red);
      const float meanP = cs * sumP * inv_n;
      const float ctc = __builtin_amdgcn_rcpf(limit_scaling(fmaxf(meanP, limit_scaling(qm[0]))));
      qv *= ctc;
      qsv *= ctc;
      cs *= ctc;
      cnP = cn2 * cs;
    }
  }
  const float cinv = 1.0f / cs;
#pragma unroll
  for (int i = 0; i < 5; ++i) {  // E scaling keeps 0 and inf
    L.lo[i] *= L.E[i];
    L.up[i] *= L.E[i];
  }
  // OSQP set_rho_vec: only a z row with fz_max - fz_min < RHO_TOL is an equality
  const bool eq4 = valid && (L.up[4] - L.lo[4] < 1e-4f);
  __syncthreads();
  if (h == 0) S.Dc[r] = valid ? Dr : 1.0f;
  // ||D^-1 q||_inf and ||q||_inf (scaled) are constant over the iterations
  float qn[2] = {fabsf(qv / Dr), fabsf(qv)};
  bmax<8, 2>(qn, S.red);  // (synchronises: S.Dc is complete after it)

  float rho = fminf(fmaxf(p_same ? prec[NP] : a.rho, 1e-6f), 1e6f), rvi = 1.0f / rho;
  const float alpha = a.alpha, oma = 1.0f - a.alpha, sigma = a.sigma;
  const int ctm = a.check_termination;
  const int interval = (a.adaptive_rho && a.rho_interval == 0)
                           ? (ctm ? 4 * ctm : 100)
                           : (a.adaptive_rho ? a.rho_interval : 0);
  int status = QLOCO_MAX_ITER, iter = 0, rho_updates = 0;
  float x = 0.0f, px = 0.0f;
  bool have_px = false, first = true;

  // the leg's x / y / z entries of a per-variable LDS vector (after a barrier)
  auto leg3 = [&](const float *v, float &vx, float &vy, float &vz) {
    vx = valid ? v[3 * pl] : 0.0f;
    vy = valid ? v[3 * pl + 1] : 0.0f;
    vz = valid ? v[3 * pl + 2] : 0.0f;
  };

  // residual norms (OSQP update_info), all threads participate; o / rr as in
  // srbd_admm_kernel's residuals()
  auto residuals = [&](float (&o)[6], float (&rr)[6], bool want_r) {
    __syncthreads();  // readers of xs / ex / err / Wc from their last use are done
    if (h == 0) {
      S.xs[r] = valid ? x * Dr : 0.0f;
      S.ex[r] = valid ? x : 0.0f;
    }
    __syncthreads();
    const float pxo = big_p_times_x(S, N, valid, step, comp, lo, hi, r2v, x * Dr, dtm, dt2m);
    px = cs * Dr * pxo;
    float xx, xy, xz;
    leg3(S.ex, xx, xy, xz);
    float aty;
    if (comp == 0) aty = L.ao[0] * L.y[0] + L.ao[1] * L.y[1];
    else if (comp == 1) aty = L.ao[2] * L.y[2] + L.ao[3] * L.y[3];
    else aty = (L.az[0] * L.y[0] + L.az[1] * L.y[1]) + (L.az[2] * L.y[2] + L.az[3] * L.y[3]) + L.ao[4] * L.y[4];
    aty = valid ? aty : 0.0f;
    const float rd = valid ? (qv + px + aty) : 0.0f;
    float e0 = 0.f, e1 = 0.f, e2 = 0.f, u0 = 0.f, u1 = 0.f, u2 = 0.f;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const float xo = i < 2 ? xx : (i < 4 ? xy : xz);
      const float ax = L.ao[i] * xo + (i < 4 ? L.az[i] * xz : 0.0f);
      const float rp = ax - L.z[i];
      const float ei = __builtin_amdgcn_rcpf(L.E[i]);
      e0 = fmaxf(e0, fabsf(ei * rp));
      e1 = fmaxf(e1, fabsf(ei * L.z[i]));
      e2 = fmaxf(e2, fabsf(ei * ax));
      u0 = fmaxf(u0, fabsf(rp));
      u1 = fmaxf(u1, fabsf(L.z[i]));
      u2 = fmaxf(u2, fabsf(ax));
    }
    const float Dinv = __builtin_amdgcn_rcpf(Dr);
    o[0] = e0;
    o[1] = e1;
    o[2] = e2;
    o[3] = fabsf(Dinv * rd);
    o[4] = fabsf(Dinv * aty);
    o[5] = fabsf(Dinv * px);
    bmax<8, 6>(o, S.red);
    if (want_r) {
      rr[0] = u0;
      rr[1] = u1;
      rr[2] = u2;
      rr[3] = fabsf(rd);
      rr[4] = fabsf(aty);
      rr[5] = fabsf(px);
      bmax<8, 6>(rr, S.red);
    }
  };

  // One code path for the first factorisation and every adaptive-rho
  // refactorisation: K = cs D P D + sigma I + A' diag(rho) A -> K^-1 -> ADMM.
  for (;;) {
    const float r4 = eq4 ? 1e3f * rho : rho, r4i = eq4 ? 1e-3f * rvi : rvi;
    {
      // this row of the leg block A' diag(rho) A (+ sigma on the diagonal)
      float add0, add1, add2;
      if (comp == 0) {
        add0 = rho * L.ao[0] * L.ao[0] + rho * L.ao[1] * L.ao[1] + sigma;
        add1 = 0.0f;
        add2 = rho * L.ao[0] * L.az[0] + rho * L.ao[1] * L.az[1];
      } else if (comp == 1) {
        add0 = 0.0f;
        add1 = rho * L.ao[2] * L.ao[2] + rho * L.ao[3] * L.ao[3] + sigma;
        add2 = rho * L.ao[2] * L.az[2] + rho * L.ao[3] * L.az[3];
      } else {
        add0 = rho * L.az[0] * L.ao[0] + rho * L.az[1] * L.ao[1];
        add1 = rho * L.az[2] * L.ao[2] + rho * L.az[3] * L.ao[3];
        add2 = (rho * L.az[0] * L.az[0] + rho * L.az[1] * L.az[1]) +
               (rho * L.az[2] * L.az[2] + rho * L.az[3] * L.az[3]) + r4 * L.ao[4] * L.ao[4] + sigma;
      }
      if (!valid) add0 = add1 = add2 = 0.0f;
      const float rs = cs * S.Dc[r];
      const float *dh = &S.Dc[HC * h];
      int lb = 3 * pl - HC * h;  // own leg's first column, relative to this half
      asm volatile("" : "+v"(lb));
#pragma unroll
      for (int c = 0; c < HC; ++c) {
        const int o = c - lb;
        const float ad = o == 0 ? add0 : (o == 1 ? add1 : (o == 2 ? add2 : 0.0f));
        K[c] = fmaf(K[c] * rs, dh[c], ad);
      }
      // Gauss-Jordan inverse (see invert_w1 for the update form), pivots in
      // the order k = HC hp + j for j = 0.., hp = 0, 1: processed(c) <=>
      // rank(c) = 2 (c mod HC) + c div HC < rank(k)
      int cnt = 0;
      const int rrank = 2 * (r % HC) + r / HC;
#pragma unroll
      for (int j = 0; j < HC; ++j) {
#pragma unroll 1
        for (int hp = 0; hp < 2; ++hp) {
          const int k = HC * hp + j;
          if (k >= n) continue;  // block-uniform
          const int buf = cnt & 1;
          ++cnt;
          if (h == hp) {
            const float v = K[j];
            S.bc[buf][r] = (r == k) ? v + 1.0f : ((rrank < 2 * j + hp) ? -v : v);  // A_kr
            S.colv[buf][r] = v;
          }
          __syncthreads();
          const float p = S.colv[buf][k];
          const float pinv = __builtin_amdgcn_rcpf(p);
          const float ng = (r == k) ? (pinv - 1.0f) : -(S.colv[buf][r] * pinv);
          const f4v *row = reinterpret_cast<const f4v *>(&S.bc[buf][HC * h]);
#pragma unroll
          for (int c4 = 0; c4 < HC / 4; ++c4) {
            const f4v bcv = row[c4];
            K[4 * c4 + 0] = fmaf(ng, bcv.x, K[4 * c4 + 0]);
            K[4 * c4 + 1] = fmaf(ng, bcv.y, K[4 * c4 + 1]);
            K[4 * c4 + 2] = fmaf(ng, bcv.z, K[4 * c4 + 2]);
            K[4 * c4 + 3] = fmaf(ng, bcv.w, K[4 * c4 + 3]);
          }
          // column k exactly for a large pivot (invert_w1)
          if (h == hp && p > kGjExactPivot) K[j] = (r == k) ? pinv : ng;
        }
      }
      __syncthreads();
    }
    if (first) {
      first = false;
      // opaque offsets per block: the record / warm-buffer addresses are
      // formed here, not kept live (64-bit each) from the entry's record read
      int vidx_f = vidx, rowbase_f = rowbase;
      asm volatile("" : "+v"(vidx_f), "+v"(rowbase_f));
      if (p_same) {
        const int vidx = vidx_f, rowbase = rowbase_f;
        // live workspace (osqp_solve without cold start): the scaled iterates as they are
        x = valid ? prec[vidx] : 0.0f;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
          L.z[i] = valid ? prec[12 * N + rowbase + i] : 0.0f;
          L.y[i] = valid ? prec[32 * N + rowbase + i] : 0.0f;
        }
      } else if (WS && (a.warm_start == 1 || p_init)) {
        const int vidx = vidx_f, rowbase = rowbase_f;
        // osqp_warm_start from the unscaled x | y: x by D^-1, y by E^-1 c, z = A x
        const float *wx = a.warm_start == 1 ? a.warm + b * (32 * N) : prec + 52 * N;
        const float *wy = wx + 12 * N;
        x = valid ? wx[vidx] / Dr : 0.0f;
#pragma unroll
        for (int i = 0; i < 5; ++i) L.y[i] = valid ? wy[rowbase + i] / L.E[i] * cs : 0.0f;
        if (h == 0) S.ex[r] = x;
        __syncthreads();
        float xx, xy, xz;
        leg3(S.ex, xx, xy, xz);
#pragma unroll
        for (int i = 0; i < 5; ++i) {
          const float xo = i < 2 ? xx : (i < 4 ? xy : xz);
          L.z[i] = L.ao[i] * xo + (i < 4 ? L.az[i] * xz : 0.0f);
        }
      }
    }
    bool refactor = false;
    while (iter < a.max_iter) {
      int next = a.max_iter;
      if (ctm) next = min(next, (iter / ctm + 1) * ctm);
      if (interval) next = min(next, (iter / interval + 1) * interval);
      for (; iter < next; ++iter) {
        // rhs = sigma x - q + A'(rho z - y)   (compute_rhs)
        float w[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) w[i] = fmaf(i == 4 ? r4 : rho, L.z[i], -L.y[i]);
        float at;
        if (comp == 0) at = L.ao[0] * w[0] + L.ao[1] * w[1];
        else if (comp == 1) at = L.ao[2] * w[2] + L.ao[3] * w[3];
        else at = (L.az[0] * w[0] + L.az[1] * w[1]) + (L.az[2] * w[2] + L.az[3] * w[3]) + L.ao[4] * w[4];
        const float rhs = valid ? fmaf(sigma, x, at - qv) : 0.0f;
        if (h == 0) S.rhs[r] = rhs;
        __syncthreads();
        // x_tilde = K^-1 rhs: this column half's partial sum
        float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;
        {
          const f4v *rv = reinterpret_cast<const f4v *>(&S.rhs[HC * h]);
#pragma unroll
          for (int c4 = 0; c4 < HC / 4; ++c4) {
            const f4v v4 = rv[c4];
            acc0 = fmaf(K[4 * c4 + 0], v4.x, acc0);
            acc1 = fmaf(K[4 * c4 + 1], v4.y, acc1);
            acc2 = fmaf(K[4 * c4 + 2], v4.z, acc2);
            acc3 = fmaf(K[4 * c4 + 3], v4.w, acc3);
          }
        }
        S.part[h][r] = (acc0 + acc1) + (acc2 + acc3);
        __syncthreads();
        float xtx = 0.f, xty = 0.f, xtz = 0.f;
        if (valid) {
          xtx = S.part[0][3 * pl] + S.part[1][3 * pl];
          xty = S.part[0][3 * pl + 1] + S.part[1][3 * pl + 1];
          xtz = S.part[0][3 * pl + 2] + S.part[1][3 * pl + 2];
        }
        const float xto = comp == 0 ? xtx : (comp == 1 ? xty : xtz);
        // update_x / update_z / update_y (relaxation alpha, projection on [l, u])
        x = fmaf(alpha, xto, oma * x);
#pragma unroll
        for (int i = 0; i < 5; ++i) {
          const float xo = i < 2 ? xtx : (i < 4 ? xty : xtz);
          const float zt = i < 4 ? fmaf(L.az[i], xtz, L.ao[i] * xo) : L.ao[i] * xo;
          const float zr = fmaf(alpha, zt, oma * L.z[i]);
          const float v = fmaf(L.y[i], i == 4 ? r4i : rvi, zr);
          const float zn = __builtin_amdgcn_fmed3f(v, L.lo[i], L.up[i]);
          L.y[i] = fmaf(i == 4 ? r4 : rho, zr - zn, L.y[i]);
          L.z[i] = zn;
        }
      }
      const bool can_check = ctm && (iter % ctm == 0);
      const bool do_rho = interval && (iter % interval == 0);
      if (can_check || do_rho) {
        float o[6], rr[6];
        residuals(o, rr, do_rho);
        have_px = true;
        const float pri_res = o[0], dua_res = cinv * o[3];
        if (can_check) {
          const float eps_p = a.eps_abs + a.eps_rel * fmaxf(o[1], o[2]);
          const float eps_d = a.eps_abs + a.eps_rel * cinv * fmaxf(fmaxf(qn[0], o[4]), o[5]);
          if (pri_res < eps_p && dua_res < eps_d) {
            status = QLOCO_OK;
            break;
          }
        }
        if (do_rho) {  // compute_rho_estimate + adapt_rho
          const float pn = rr[0] / (fmaxf(rr[1], rr[2]) + 1e-30f);
          const float dn = rr[3] / (fmaxf(fmaxf(qn[1], rr[4]), rr[5]) + 1e-30f);
          float rho_new = rho * sqrtf(pn / (dn + 1e-30f));
          rho_new = fminf(fmaxf(rho_new, 1e-6f), 1e6f);
          if (rho_new > rho * a.rho_tol || rho_new < rho / a.rho_tol) {
            rho = rho_new;
            rvi = 1.0f / rho;
            rho_updates++;
            refactor = true;
            break;
          }
        }
      }
    }
    if (!refactor) break;
    big_p_row(S, lo, hi, r, h, valid, step, comp, r2v, dtm, dt2m, K);
  }
  if (status != QLOCO_OK) {  // max_iter reached (OSQP: solved inaccurate or max_iter)
    float o[6], rr[6];
    residuals(o, rr, false);
    have_px = true;
    const float pri_res = o[0], dua_res = cinv * o[3];
    const float ep = 10.f * a.eps_abs + 10.f * a.eps_rel * fmaxf(o[1], o[2]);
    const float ed = 10.f * a.eps_abs + 10.f * a.eps_rel * cinv * fmaxf(fmaxf(qn[0], o[4]), o[5]);
    status = (pri_res < ep && dua_res < ed) ? QLOCO_SOLVED_INACCURATE : QLOCO_MAX_ITER;
  }

  // ---------------- 8. outputs: unscale, objective, scatter to leg slots
  if (!have_px) {  // max_iter == 0
    float o[6], rr[6];
    residuals(o, rr, false);
  }
  const float xu = valid ? x * Dr : 0.0f;
  const float objp = bsum<8>((valid && h == 0) ? cinv * (0.5f * x * px + qv * x) : 0.0f, S.red);
  const bool bad = !isfinite(objp);
  if (bad) status = QLOCO_NAN;
  if (a.u) {  // full solution (world frame), swing forces exactly 0
    float *uo = a.u + b * 12 * N;
    for (int k = t; k < 12 * N; k += kBigThreads) uo[k] = 0.0f;
    __syncthreads();
    if (valid && h == 0) uo[vidx] = bad ? NAN : xu;
  }
  __syncthreads();
  if (h == 0) S.xs[r] = xu;
  __syncthreads();
  if (t < 12) {  // u0: step-0 forces; optional body frame R' u (A1RobotControl.cpp:596-599)
    const int lg = t / 3, cp = t - 3 * lg;
    float f0 = 0.f, f1 = 0.f, f2 = 0.f;
    for (int p = 0; p < S.stepstart[1]; ++p) {
      if ((S.legtab[p] & 3) == lg) {
        f0 = S.xs[3 * p];
        f1 = S.xs[3 * p + 1];
        f2 = S.xs[3 * p + 2];
      }
    }
    float o = cp == 0 ? f0 : (cp == 1 ? f1 : f2);
    if (a.output_frame == 1)  // R^T f with R = [[c,s,0],[-s,c,0],[0,0,1]]
      o = cp == 0 ? (R00 * f0 + R10 * f1) : (cp == 1 ? (R01 * f0 + R11 * f1) : f2);
    a.u0[b * 12 + t] = bad ? NAN : o;
  }
  if (prec) {  // the persistent record for the next call (layout: srbd_admm_kernel)
    for (int k = t; k < NP + 4; k += kBigThreads) prec[k] = 0.0f;
    __syncthreads();
    int vidx_o = vidx, rowbase_o = rowbase;
    asm volatile("" : "+v"(vidx_o), "+v"(rowbase_o));
    const int vidx = vidx_o, rowbase = rowbase_o;
    if (valid && h == 0) {
      prec[vidx] = x;
      prec[52 * N + vidx] = xu;
      prec[84 * N + vidx] = q_raw;
      if (comp == 0) {  // the leg's rows, once
#pragma unroll
        for (int i = 0; i < 5; ++i) {
          prec[12 * N + rowbase + i] = L.z[i];
          prec[32 * N + rowbase + i] = L.y[i];
          prec[64 * N + rowbase + i] = cinv * L.E[i] * L.y[i];
        }
      }
    }
    for (int k = t; k < 4 * N; k += kBigThreads) prec[96 * N + k] = S.ct[k] ? 1.0f : 0.0f;
    if (t == 0) {
      prec[NP] = rho;
      prec[NP + 1] = 1.0f;
    }
  }
  if (WS && a.warm_start == 1) {
    const int nu = 12 * N, ncn = 20 * N;
    float *wx = a.warm + b * (nu + ncn);
    float *wy = wx + nu;
    for (int k = t; k < nu + ncn; k += kBigThreads) wx[k] = 0.0f;
    __syncthreads();
    int vidx_o = vidx, rowbase_o = rowbase;
    asm volatile("" : "+v"(vidx_o), "+v"(rowbase_o));
    const int vidx = vidx_o, rowbase = rowbase_o;
    if (valid && h == 0) {
      wx[vidx] = xu;
      if (comp == 0) {
#pragma unroll
        for (int i = 0; i < 5; ++i) wy[rowbase + i] = cinv * L.E[i] * L.y[i];
      }
    }
  }
  if (t == 0) {
    if (a.status) a.status[b] = status;
    if (a.iters) a.iters[b] = iter;
    if (a.rho_updates) a.rho_updates[b] = rho_updates;
    if (a.obj) a.obj[b] = objp;
  }
}

}  // namespace qloco

// qloco_force_qp.inc -- the statements of the Go1 force-QP kernel, included by
// qloco_force.hip into force_qp_kernel<GW> (Rows = false) and
// force_qp_body_kernel<GW> (Rows = true).  Text and not a function: with the
// body in a __forceinline__ function and the kernels as wrappers, the compiler
// schedules the kernel-argument loads differently (force_qp_kernel<16>: 242
// VGPRs against 240, more than a third of the instructions changed), and
// force_qp_kernel without rows must stay, instruction for instruction, the
// kernel it was.
// The including kernel provides: GW, `constexpr bool Rows`, `const ForceArgs a`
// and `const qloco_force_body *rows` (unused without Rows).
//
// Rows = true: robot inst takes alpha, beta, gamma, fz_max, mu from rows[inst].
// The group stages the row's 16 doubles in J (free until G is built), every
// lane applies force_body_ok to them, and the five values -- the row's, or the
// kernel arguments' as a stand-in when the row is refused, so that the group
// walks the same code beside its neighbours -- go to the group's slot of Q.  A
// refused robot stores nothing but its refusal.
  constexpr int FG = 64 / GW, VL = (12 + GW - 1) / GW;
  __shared__ ForceLds<FG> S;
  const int lane = threadIdx.x, grp = lane / GW, li = lane % GW;
  const int64_t pos = (int64_t)blockIdx.x * FG + grp;
  if (pos >= a.batch) return;
  const int64_t inst = a.list ? a.list[pos] : pos;
  typename ForceLds<FG>::Grp &P = S.g[grp];
  double *const PA = P.gi.R;  // A, 6x12 col-major (dead before the solver clears R)
  double *const PG = P.gi.J;  // G, 12x12 col-major (read once, before J is formed)
  static_assert(sizeof(P.gi.R) >= 72 * sizeof(double), "A fits the packed R");
  double *const Pg0 = P.gi.z;  // g0 (dead before z is first written)
  bool refused = false;
  const double *q = nullptr;
  if constexpr (Rows) {
    const double *src = reinterpret_cast<const double *>(rows + inst);
#pragma unroll
    for (int k = li; k < 16; k += GW) PG[k] = src[k];
    GI_SYNC();
    refused = !force_body_ok(PG);
    __shared__ ForceBodyLds<FG> Q;
    double *const w = Q.q[grp];
    // slot entry k = row double k + 1 (alpha .. mu); the stand-in by a static
    // select chain over the kernel arguments
    const double arg = li == 0 ? a.alpha : li == 1 ? a.beta : li == 2 ? a.gamma : li == 3 ? a.fz_max : a.mu;
    if (li < 5) w[li] = refused ? arg : PG[li + 1];
    GI_SYNC();
    q = w;
  }
  // alpha, beta, gamma: kernel arguments, or read from the slot where they are used
  auto alpha = [&]() { if constexpr (Rows) return q[0]; else return a.alpha; };
  auto beta = [&]() { if constexpr (Rows) return q[1]; else return a.beta; };
  auto gamma = [&]() { if constexpr (Rows) return q[2]; else return a.gamma; };

  // ---- force_distribution (state F_leg_ref in/out) -> F_leg_guess
  double Fref[12];
  for (int k = 0; k < 12; ++k) Fref[k] = a.F_leg_ref[inst * 12 + k];
  force_distribution(a.com_des + inst * 3, a.leg_des + inst * 12, a.F_force_des + inst * 6,
                     a.mode[inst], a.y_coef[inst], a.rfoot_des + inst * 3, a.lfoot_des + inst * 3,
                     Fref);
  // this lane's entries by a static select chain: indexing Fref by li would put
  // the array in scratch (a per-lane spill of 96 B, written back to HBM)
  double guess[VL];  // F_leg_guess entries li + GW v (only their lane reads them)
#pragma unroll
  for (int v = 0; v < VL; ++v) {
    guess[v] = Fref[0];
#pragma unroll
    for (int k = 1; k < 12; ++k) guess[v] = (li + GW * v == k) ? Fref[k] : guess[v];
  }
  // ---- force_opt: A (6x12, col-major) with the skew_hat quirk (:274-298)
#pragma unroll
  for (int v = 0; v < VL; ++v) {
    const int r = li + GW * v;
    if (r < 12)
      for (int k = 0; k < 6; ++k) PA[r * 6 + k] = 0.0;
  }
  GI_SYNC();
  if (li < 4) {
    const int leg = li;
    const double *bp = a.base_p + inst * 3;
    const double *fp = a.feet_p + inst * 12 + 3 * leg;
    const double v0 = bp[0] - fp[0];  // skew_hat uses vec_w[0] everywhere (comma operator)
    for (int k = 0; k < 3; ++k) PA[(3 * leg + k) * 6 + k] = 1.0;
    // W rows [0,-a,a],[a,0,-a],[-a,a,0]
    const double W[3][3] = {{0.0, -v0, v0}, {v0, 0.0, -v0}, {-v0, v0, 0.0}};
    for (int r = 0; r < 3; ++r)
      for (int k = 0; k < 3; ++k) PA[(3 * leg + k) * 6 + 3 + r] = W[r][k];
  }
  GI_SYNC();
  // G = 2 (alpha A'A + (beta+gamma) I), then (G' + G)/2 ; g0 (:300-305).
  // A'A(r,c) and A'A(c,r) are the same products summed in the same order, so G
  // is exactly symmetric and (G' + G)/2 = (x + x)/2 = x bit for bit: the
  // symmetrisation is the identity and is not executed.
#pragma unroll
  for (int v = 0; v < VL; ++v) {
    const int r = li + GW * v;
    if (r < 12) {
      for (int c = 0; c < 12; ++c) {
        double ata = 0.0;
        for (int k = 0; k < 6; ++k) ata += PA[r * 6 + k] * PA[c * 6 + k];
        PG[c * 12 + r] = 2.0 * (alpha() * ata + (r == c ? (beta() + gamma()) : 0.0));
      }
    }
  }
  GI_SYNC();
#pragma unroll
  for (int v = 0; v < VL; ++v) {
    const int r = li + GW * v;
    if (r < 12) {
      double atf = 0.0;
      const double *FT = a.FT_total_des + inst * 6;
      for (int k = 0; k < 6; ++k) atf += PA[r * 6 + k] * FT[k];
      const double prev = a.grf_opt[inst * 12 + r];
      Pg0[r] = -2.0 * (alpha() * atf + beta() * guess[v] + gamma() * prev);
      // _X = grf_opt (:391).  A failed Cholesky leaves the solver before it
      // forms x (EiQuadProg.cpp:505-510) and the core then hands back what
      // gi.x held: seeded, that is the carried grf_opt -- the reference's
      // result -- and not LDS this block never wrote.
      P.gi.x[r] = prev;
    }
  }
  GI_SYNC();
  // swing-leg equality pattern AA (:310-350)
  const int pat = force_pattern(a.mode[inst], a.right_support[inst]);
  double f;
  int st, it;
  if constexpr (Rows)
    gi_solve_group<GW>(P.gi, li, 12, 12, 24, PG, 12, Pg0, c_force_CE[pat], c_force_zeros,
                       ForceCiRow{q}, P.gi.x, f, st, it);
  else
  gi_solve_group<GW>(P.gi, li, 12, 12, 24, PG, 12, Pg0, c_force_CE[pat], c_force_zeros,
                 ForceCi{a.mu, a.fz_max}, P.gi.x,
                 f, st, it);
  GI_SYNC();
  if constexpr (Rows) if (refused) {  // the stand-in's solve is not this robot's: the member state
                          // (F_leg_ref, grf_opt, the iteration count) stays as it was
#pragma unroll
    for (int v = 0; v < VL; ++v) {
      const int r = li + GW * v;
      if (r < 12) a.F_leg_guess[inst * 12 + r] = __longlong_as_double(0x7ff8000000000000ll);
    }
    if (li == 0) {
      if (a.qp_solution) a.qp_solution[inst] = 0;
      if (a.status) a.status[inst] = QLOCO_ERR_ARG;
      if (a.iters) a.iters[inst] = 0;
    }
    return;
  }
  // QPBaseClass::solveQP: success iff no NaN (go1_rt_control QPBaseClass.cpp:116-142); Solve / fallback
  bool ok = true;
  for (int k = 0; k < 12; ++k) ok = ok && !isnan(P.gi.x[k]);
#pragma unroll
  for (int v = 0; v < VL; ++v) {
    const int r = li + GW * v;
    if (r < 12) {
      a.grf_opt[inst * 12 + r] = ok ? P.gi.x[r] : guess[v];
      a.F_leg_guess[inst * 12 + r] = guess[v];
      a.F_leg_ref[inst * 12 + r] = guess[v];  // = Fref (F_leg_guess := F_leg_ref, :251-260)
    }
  }
  if (li == 0) {
    if (a.qp_solution) a.qp_solution[inst] = ok ? 1 : 0;
    if (a.status) a.status[inst] = st;
    if (a.iters) a.iters[inst] = it;
    if (a.prev_it) a.prev_it[inst] = it;
  }

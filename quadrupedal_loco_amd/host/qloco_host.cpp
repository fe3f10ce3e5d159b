// qloco_host.cpp -- C++ host shim (include/qloco.hpp) over the C ABI.
//
// Host code only: it stages reference-shaped host arrays to the device on a
// HIP stream and calls libqloco.so.  No solver arithmetic lives here except
// the reference's own input assembly for compute_grf
// (A1RobotControl.cpp:459-497), which is host-side in the reference too.
#include <algorithm>

#include "qloco.hpp"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>

namespace qloco {

Error::Error(const std::string &what, int s) : std::runtime_error(what), status(s) {}

static void hip_ok(hipError_t e, const char *where) {
  if (e != hipSuccess)
    throw Error(std::string(where) + ": " + hipGetErrorString(e), QLOCO_ERR_DEVICE);
}
static void abi_ok(int s, const char *where) {
  if (s != QLOCO_OK)
    throw Error(std::string(where) + " failed: " + qloco_status_string(s) + " " +
                    qloco_last_error(),
                s);
}

// ---------------------------------------------------------------- DeviceArena
DeviceArena::DeviceArena() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
    throw Error("qloco: no GPU visible (the solver has no CPU fallback)", QLOCO_ERR_NO_GPU);
  hipStream_t s;
  hip_ok(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreate");
  stream_ = s;
}
DeviceArena::~DeviceArena() {
  for (void *p : blocks_) (void)hipFree(p);
  if (stream_) (void)hipStreamDestroy((hipStream_t)stream_);
}
void *DeviceArena::alloc(size_t bytes) {
  void *p = nullptr;
  hip_ok(hipMalloc(&p, bytes ? bytes : 16), "hipMalloc");
  blocks_.push_back(p);
  return p;
}
void DeviceArena::release(void *p) {
  if (!p) return;
  for (size_t i = 0; i < blocks_.size(); ++i)
    if (blocks_[i] == p) {
      (void)hipFree(p);
      blocks_[i] = blocks_.back();
      blocks_.pop_back();
      return;
    }
}
void DeviceArena::upload(void *dev, const void *host, size_t bytes) {
  if (bytes) hip_ok(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, (hipStream_t)stream_), "upload");
}
void DeviceArena::download(void *host, const void *dev, size_t bytes) {
  if (bytes) hip_ok(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream_), "download");
}
void DeviceArena::sync() { hip_ok(hipStreamSynchronize((hipStream_t)stream_), "hipStreamSynchronize"); }

template <class T>
static T *dalloc(DeviceArena &a, size_t n) {
  return static_cast<T *>(a.alloc(n * sizeof(T)));
}

// ---------------------------------------------------------------- QPsolverGpu
QPsolverGpu::QPsolverGpu(int max_batch) : max_batch_(max_batch < 1 ? 1 : max_batch) {}
QPsolverGpu::~QPsolverGpu() = default;

void QPsolverGpu::resize(const int &nVar, const int &nEq, const int &nIneq) {
  // QPBaseClass.cpp:111-112 asserts nVars <= 60, nIneq <= 300; the kernels
  // take n, p <= 64, m <= 320 (qloco_gi_limits)
  int32_t ln = 0, lp = 0, lm = 0;
  qloco_gi_limits(&ln, &lp, &lm);
  if (nVar < 1 || nVar > ln || nEq < 0 || nEq > lp || nIneq < 0 || nIneq > lm)
    throw Error("QPsolverGpu::resize: size out of range", QLOCO_BAD_SIZE);
  n_ = nVar;
  p_ = nEq;
  m_ = nIneq;
}

// Device blocks are reused while the batch and the (n, p, m) of the last
// resize fit the sizes they were allocated for; otherwise the old blocks are
// freed before the new ones are allocated (repeated resizeQP calls or a
// growing batch do not accumulate device memory).
void QPsolverGpu::ensure(int batch) {
  if (batch <= cap_ && n_ <= an_ && p_ <= ap_ && m_ <= am_) return;
  for (void *p : {(void *)dG_, (void *)dg0_, (void *)dCE_, (void *)dce0_, (void *)dCI_,
                  (void *)dci0_, (void *)dX_, (void *)df_, (void *)dst_, (void *)dit_})
    arena_.release(p);
  dG_ = dg0_ = dCE_ = dce0_ = dCI_ = dci0_ = dX_ = df_ = nullptr;
  dst_ = dit_ = nullptr;
  if (batch < cap_) batch = cap_;
  const size_t B = batch;
  dG_ = dalloc<double>(arena_, B * n_ * n_);
  dg0_ = dalloc<double>(arena_, B * n_);
  dCE_ = dalloc<double>(arena_, B * (p_ ? n_ * p_ : 1));
  dce0_ = dalloc<double>(arena_, B * (p_ ? p_ : 1));
  dCI_ = dalloc<double>(arena_, B * (m_ ? n_ * m_ : 1));
  dci0_ = dalloc<double>(arena_, B * (m_ ? m_ : 1));
  dX_ = dalloc<double>(arena_, B * n_);
  df_ = dalloc<double>(arena_, B);
  dst_ = dalloc<int32_t>(arena_, B);
  dit_ = dalloc<int32_t>(arena_, B);
  cap_ = batch;
  an_ = n_;
  ap_ = p_;
  am_ = m_;
}

void QPsolverGpu::solve_batch(int batch, const double *G, const double *g0, const double *CE,
                              const double *ce0, const double *CI, const double *ci0,
                              double *X, double *f, int32_t *status) {
  if (n_ == 0) throw Error("QPsolverGpu: resize() first", QLOCO_ERR_ARG);
  ensure(batch);
  const size_t B = batch;
  arena_.upload(dG_, G, sizeof(double) * B * n_ * n_);
  arena_.upload(dg0_, g0, sizeof(double) * B * n_);
  if (p_) {
    arena_.upload(dCE_, CE, sizeof(double) * B * n_ * p_);
    arena_.upload(dce0_, ce0, sizeof(double) * B * p_);
  }
  if (m_) {
    arena_.upload(dCI_, CI, sizeof(double) * B * n_ * m_);
    arena_.upload(dci0_, ci0, sizeof(double) * B * m_);
  }
  abi_ok(qloco_eiquadprog_solve(n_, p_, m_, batch, dG_, (int64_t)n_ * n_, dg0_, n_,
                                p_ ? dCE_ : nullptr, (int64_t)n_ * p_, p_ ? dce0_ : nullptr, p_,
                                m_ ? dCI_ : nullptr, (int64_t)n_ * m_, m_ ? dci0_ : nullptr, m_,
                                dX_, df_, dst_, dit_, arena_.stream()),
         "qloco_eiquadprog_solve");
  arena_.download(X, dX_, sizeof(double) * B * n_);
  std::vector<double> fh(B);
  std::vector<int32_t> sh(B), ih(B);
  arena_.download(fh.data(), df_, sizeof(double) * B);
  arena_.download(sh.data(), dst_, sizeof(int32_t) * B);
  arena_.download(ih.data(), dit_, sizeof(int32_t) * B);
  arena_.sync();
  if (f) std::memcpy(f, fh.data(), sizeof(double) * B);
  if (status) std::memcpy(status, sh.data(), sizeof(int32_t) * B);
  last_status_ = sh[B - 1];
  last_iters_ = ih[B - 1];
}

double QPsolverGpu::solve(const double *G, const double *g0, const double *CE, const double *ce0,
                          const double *CI, const double *ci0, double *X) {
  double f = 0.0;
  solve_batch(1, G, g0, CE, ce0, CI, ci0, X, &f, nullptr);
  return f;
}

void QPBaseClassGpu::resizeQP(const int &nv, const int &ne, const int &ni) {
  nVars = nv;
  nEq = ne;
  nIneq = ni;
  G.assign((size_t)nv * nv, 0.0);
  g0.assign(nv, 0.0);
  CE.assign((size_t)nv * ne, 0.0);
  ce0.assign(ne, 0.0);
  CI.assign((size_t)nv * ni, 0.0);
  ci0.assign(ni, 0.0);
  X.assign(nv, 0.0);
  solver_.resize(nv, ne, ni);
}

bool QPBaseClassGpu::solveQP() {  // QPBaseClass.cpp:126-152
  solver_.solve(G.data(), g0.data(), CE.data(), ce0.data(), CI.data(), ci0.data(), X.data());
  for (double v : X)
    if (std::isnan(v)) return false;
  return true;
}

// ---------------------------------------------------------------- Dynamiccclass
Dynamiccclass::Dynamiccclass(int batch, const qloco_force_params *params) : batch_(batch) {
  if (batch < 1) throw Error("Dynamiccclass: batch < 1", QLOCO_ERR_ARG);
  if (params) prm_ = *params;
  else qloco_force_params_default(&prm_);
  const size_t B = batch;
  grf_opt.assign(B * 12, 0.0);
  F_leg_ref.assign(B * 12, 0.0);
  F_leg_guess.assign(B * 12, 0.0);
  qp_solution.assign(B, 1);
  status.assign(B, 0);
  iters.assign(B, 0);
  h_com_.assign(B * 3, 0.0);
  h_leg_.assign(B * 12, 0.0);
  h_F_.assign(B * 6, 0.0);
  h_rf_.assign(B * 3, 0.0);
  h_lf_.assign(B * 3, 0.0);
  h_base_.assign(B * 3, 0.0);
  h_feet_.assign(B * 12, 0.0);
  h_FT_.assign(B * 6, 0.0);
  h_y_.assign(B, 0.0);
  h_mode_.assign(B, 0);
  h_rs_.assign(B, 2);
  d_com_ = dalloc<double>(arena_, B * 3);
  d_leg_ = dalloc<double>(arena_, B * 12);
  d_F_ = dalloc<double>(arena_, B * 6);
  d_rf_ = dalloc<double>(arena_, B * 3);
  d_lf_ = dalloc<double>(arena_, B * 3);
  d_base_ = dalloc<double>(arena_, B * 3);
  d_feet_ = dalloc<double>(arena_, B * 12);
  d_FT_ = dalloc<double>(arena_, B * 6);
  d_y_ = dalloc<double>(arena_, B);
  d_Fref_ = dalloc<double>(arena_, B * 12);
  d_grf_ = dalloc<double>(arena_, B * 12);
  d_guess_ = dalloc<double>(arena_, B * 12);
  d_mode_ = dalloc<int32_t>(arena_, B);
  d_rs_ = dalloc<int32_t>(arena_, B);
  d_qps_ = dalloc<int32_t>(arena_, B);
  d_st_ = dalloc<int32_t>(arena_, B);
  d_it_ = dalloc<int32_t>(arena_, B);
  // the grouped launch's workspace (previous iteration counts carried between calls)
  const size_t nord = (size_t)qloco_force_order_ws_len(batch);
  d_ord_ = dalloc<int32_t>(arena_, nord);
  hip_ok(hipMemsetAsync(d_ord_, 0, sizeof(int32_t) * nord, (hipStream_t)arena_.stream()), "order workspace");
  // member state starts at zero (Dynamiccclass ctor, dynmics_compute.cpp:29-100)
  arena_.upload(d_Fref_, F_leg_ref.data(), sizeof(double) * B * 12);
  arena_.upload(d_grf_, grf_opt.data(), sizeof(double) * B * 12);
  arena_.sync();
}

void Dynamiccclass::force_distribution(const double com_des[3], const double leg_des[12],
                                       const double F_force_des[6], int mode,
                                       double y_coefficient, const double rfoot_des[3],
                                       const double lfoot_des[3], int r) {
  if (r < 0 || r >= batch_) throw Error("Dynamiccclass: robot index", QLOCO_ERR_ARG);
  std::memcpy(&h_com_[r * 3], com_des, sizeof(double) * 3);
  std::memcpy(&h_leg_[r * 12], leg_des, sizeof(double) * 12);
  std::memcpy(&h_F_[r * 6], F_force_des, sizeof(double) * 6);
  std::memcpy(&h_rf_[r * 3], rfoot_des, sizeof(double) * 3);
  std::memcpy(&h_lf_[r * 3], lfoot_des, sizeof(double) * 3);
  h_mode_[r] = mode;
  h_y_[r] = y_coefficient;
}

void Dynamiccclass::force_opt(const double base_p[3], const double FR_p[3], const double FL_p[3],
                              const double RR_p[3], const double RL_p[3],
                              const double FT_total_des[6], int mode, int right_support,
                              double y_coefficient, int r) {
  if (r < 0 || r >= batch_) throw Error("Dynamiccclass: robot index", QLOCO_ERR_ARG);
  std::memcpy(&h_base_[r * 3], base_p, sizeof(double) * 3);
  std::memcpy(&h_feet_[r * 12 + 0], FR_p, sizeof(double) * 3);
  std::memcpy(&h_feet_[r * 12 + 3], FL_p, sizeof(double) * 3);
  std::memcpy(&h_feet_[r * 12 + 6], RR_p, sizeof(double) * 3);
  std::memcpy(&h_feet_[r * 12 + 9], RL_p, sizeof(double) * 3);
  std::memcpy(&h_FT_[r * 6], FT_total_des, sizeof(double) * 6);
  h_mode_[r] = mode;  // force_opt's own mode / y_coefficient arguments (:265)
  h_rs_[r] = right_support;
  h_y_[r] = y_coefficient;
  if (r == batch_ - 1) run();
}

void Dynamiccclass::run() {
  const size_t B = batch_;
  arena_.upload(d_com_, h_com_.data(), sizeof(double) * B * 3);
  arena_.upload(d_leg_, h_leg_.data(), sizeof(double) * B * 12);
  arena_.upload(d_F_, h_F_.data(), sizeof(double) * B * 6);
  arena_.upload(d_rf_, h_rf_.data(), sizeof(double) * B * 3);
  arena_.upload(d_lf_, h_lf_.data(), sizeof(double) * B * 3);
  arena_.upload(d_base_, h_base_.data(), sizeof(double) * B * 3);
  arena_.upload(d_feet_, h_feet_.data(), sizeof(double) * B * 12);
  arena_.upload(d_FT_, h_FT_.data(), sizeof(double) * B * 6);
  arena_.upload(d_y_, h_y_.data(), sizeof(double) * B);
  arena_.upload(d_mode_, h_mode_.data(), sizeof(int32_t) * B);
  arena_.upload(d_rs_, h_rs_.data(), sizeof(int32_t) * B);
  abi_ok(qloco_force_qp_solve_body(&prm_, batch_, d_com_, d_leg_, d_F_, d_rf_, d_lf_, d_base_,
                                   d_feet_, d_FT_, d_mode_, d_rs_, d_y_, d_Fref_, d_grf_, d_guess_,
                                   d_qps_, d_st_, d_it_, d_ord_, body_.get(), arena_.stream()),
         "qloco_force_qp_solve_body");
  arena_.download(grf_opt.data(), d_grf_, sizeof(double) * B * 12);
  arena_.download(F_leg_ref.data(), d_Fref_, sizeof(double) * B * 12);
  arena_.download(F_leg_guess.data(), d_guess_, sizeof(double) * B * 12);
  arena_.download(qp_solution.data(), d_qps_, sizeof(int32_t) * B);
  arena_.download(status.data(), d_st_, sizeof(int32_t) * B);
  arena_.download(iters.data(), d_it_, sizeof(int32_t) * B);
  arena_.sync();
}

void Dynamiccclass::compute_joint_torques(const double *Jaco, const int32_t *swing,
                                          const double *p_des, const double *p_est,
                                          const double *pv_des, const double *pv_est,
                                          double *tau) {
  const size_t B = batch_;
  if (!d_jt_) {
    d_jt_ = dalloc<double>(arena_, B * (36 + 48 + 12));
    d_sw_ = dalloc<int32_t>(arena_, B * 4);
  }
  double *dJ = d_jt_, *dp = d_jt_ + B * 36, *dtau = d_jt_ + B * 84;
  int32_t *dsw = d_sw_;
  arena_.upload(dJ, Jaco, sizeof(double) * B * 36);
  arena_.upload(dsw, swing, sizeof(int32_t) * B * 4);
  arena_.upload(dp, p_des, sizeof(double) * B * 12);
  arena_.upload(dp + B * 12, p_est, sizeof(double) * B * 12);
  arena_.upload(dp + B * 24, pv_des, sizeof(double) * B * 12);
  arena_.upload(dp + B * 36, pv_est, sizeof(double) * B * 12);
  abi_ok(qloco_joint_torques(batch_, dJ, dsw, dp, dp + B * 12, dp + B * 24, dp + B * 36, d_Fref_,
                             dtau, arena_.stream()),
         "qloco_joint_torques");
  arena_.download(tau, dtau, sizeof(double) * B * 12);
  arena_.sync();
}

// ---------------------------------------------------------------- PRMPCClass
PRMPCClass::PRMPCClass(int batch) : batch_(batch) {
  if (batch < 1) throw Error("PRMPCClass: batch < 1", QLOCO_ERR_ARG);
  const size_t B = batch;
  state.assign(B * QLOCO_BODY_STATE_LEN, 0.0);
  abi_ok(qloco_body_state_init_host(batch, state.data()), "qloco_body_state_init_host");
  d_state_ = dalloc<double>(arena_, B * QLOCO_BODY_STATE_LEN);
  d_in_ = dalloc<double>(arena_, B * (4 + 4 * 10 + 15));
  d_traj_ = dalloc<double>(arena_, B * 14);
  d_t_ = dalloc<double>(arena_, 1);
  d_i_ = dalloc<int32_t>(arena_, B);
  d_st_ = dalloc<int32_t>(arena_, B);
  d_j_ = dalloc<int32_t>(arena_, 1);
  arena_.upload(d_state_, state.data(), sizeof(double) * B * QLOCO_BODY_STATE_LEN);
  arena_.sync();
}

void PRMPCClass::body_theta_mpc_batch(const int32_t *i, const double *bs, const double *zmp,
                                      const double *ang, const double *rf, const double *lf,
                                      const double *acc, double *com_traj) {
  const size_t B = batch_;
  double *d_bs = d_in_, *d_zmp = d_bs + B * 4, *d_ang = d_zmp + B * 10, *d_rf = d_ang + B * 10,
         *d_lf = d_rf + B * 10, *d_acc = d_lf + B * 10;
  arena_.upload(d_i_, i, sizeof(int32_t) * B);
  arena_.upload(d_bs, bs, sizeof(double) * B * 4);
  arena_.upload(d_zmp, zmp, sizeof(double) * B * 10);
  arena_.upload(d_ang, ang, sizeof(double) * B * 10);
  arena_.upload(d_rf, rf, sizeof(double) * B * 10);
  arena_.upload(d_lf, lf, sizeof(double) * B * 10);
  arena_.upload(d_acc, acc, sizeof(double) * B * 15);
  abi_ok(qloco_body_mpc_step(batch_, d_i_, d_bs, d_zmp, d_ang, d_rf, d_lf, d_acc, d_state_,
                             d_traj_, d_st_, arena_.stream()),
         "qloco_body_mpc_step");
  arena_.download(com_traj, d_traj_, sizeof(double) * B * 14);
  arena_.download(state.data(), d_state_, sizeof(double) * B * QLOCO_BODY_STATE_LEN);
  arena_.sync();
}

std::array<double, 14> PRMPCClass::body_theta_mpc(int i, const double bodyangle_state[4],
                                                  const double zmp_ref[10],
                                                  const double angle_ref[10],
                                                  const double rfoot_ref[10],
                                                  const double lfoot_ref[10],
                                                  const double comacc_ref[15],
                                                  const double * /*Nrtfoorpr_gen*/) {
  if (batch_ != 1) throw Error("PRMPCClass::body_theta_mpc: use body_theta_mpc_batch", QLOCO_ERR_ARG);
  std::array<double, 14> out{};
  const int32_t ii = i;
  body_theta_mpc_batch(&ii, bodyangle_state, zmp_ref, angle_ref, rfoot_ref, lfoot_ref, comacc_ref,
                       out.data());
  return out;
}

int PRMPCClass::Indexfind(double goal_P) {
  int32_t j = 0;
  arena_.upload(d_t_, &goal_P, sizeof(double));
  abi_ok(qloco_body_indexfind(1, d_t_, d_j_, arena_.stream()), "qloco_body_indexfind");
  arena_.download(&j, d_j_, sizeof(int32_t));
  arena_.sync();
  return j;
}

// ---------------------------------------------------------------- ConvexMpcBatch
// argument check in the member-initialiser list: batch_ is declared before
// the DeviceArena, so a bad batch is refused before any device call
static int positive_batch(int batch, const char *who) {
  if (batch < 1) throw Error(std::string(who) + ": batch < 1", QLOCO_ERR_ARG);
  return batch;
}

ConvexMpcBatch::ConvexMpcBatch(int batch, const qloco_srbd_spec *sp)
    : batch_(positive_batch(batch, "ConvexMpcBatch")) {
  if (sp) {
    spec = *sp;
  } else {
    qloco_srbd_spec_default(&spec);
    spec.warm_start = 2;       // the reference's persistent member solver
    spec.literal_full_qp = 1;  // on its literal 12N-variable QP (update path every call)
  }
  if (spec.horizon < 1 || spec.horizon > 20)
    throw Error("ConvexMpcBatch: horizon outside 1..20", QLOCO_BAD_SIZE);
  if (spec.warm_start < 0 || spec.warm_start > 2)
    throw Error("ConvexMpcBatch: warm_start outside 0..2", QLOCO_ERR_ARG);
  // the device buffers (x_ref, the persistent record) are sized from these:
  // later edits of the public spec are checked against them on every call
  horizon_ = spec.horizon;
  warm_mode_ = spec.warm_start;
  spec.feet_per_step = 0;      // compute_grf passes one foot_pos_abs (:527-531)
  spec.contacts_per_step = 0;  // and one contacts[4] (ConvexMpc.cpp:232-249)
  spec.output_frame = 1;       // root_rot_mat' u (:596-599)
  const size_t B = batch, N = spec.horizon;
  d_x0_ = dalloc<float>(arena_, B * 13);
  d_xr_ = dalloc<float>(arena_, B * 13 * N);
  d_feet_ = dalloc<float>(arena_, B * 12);
  d_ct_ = dalloc<uint8_t>(arena_, B * 4);
  d_u0_ = dalloc<float>(arena_, B * 12);
  d_st_ = dalloc<int32_t>(arena_, B);
  d_it_ = dalloc<int32_t>(arena_, B);
  if (spec.warm_start == 2) {  // per-robot persistent solver record
    d_rec_ = dalloc<float>(arena_, B * QLOCO_SRBD_PERSIST_LEN(N));
    reset();
  }
  status.assign(B, 0);
  iters.assign(B, 0);
}

static int shard_count_of(int64_t total, int world, int rank, int mode) {
  int64_t count = 0;
  if (qloco_mgpu_shard(total, world, rank, mode, nullptr, &count, nullptr) != QLOCO_OK)
    throw Error("ConvexMpcBatch: invalid shard (total, world, rank, mode)", QLOCO_ERR_ARG);
  if (count < 1 || count > INT32_MAX)
    throw Error("ConvexMpcBatch: this rank's shard is empty or too large", QLOCO_BAD_SIZE);
  return (int)count;
}

ConvexMpcBatch::ConvexMpcBatch(int64_t total, int world, int rank, const uint8_t *comm_id,
                               int shard_mode, const qloco_srbd_spec *sp)
    : ConvexMpcBatch(shard_count_of(total, world, rank, shard_mode), sp) {
  abi_ok(qloco_mgpu_shard(total, world, rank, shard_mode, &shard_first, &shard_count, &shard_stride),
         "qloco_mgpu_shard");
  total_ = total;
  d_u0_all_ = dalloc<float>(arena_, (size_t)total * 12);
  d_st_all_ = dalloc<int32_t>(arena_, (size_t)total);
  d_it_all_ = dalloc<int32_t>(arena_, (size_t)total);
  all_forces_.assign((size_t)total * 12, 0.0);
  abi_ok(qloco_mgpu_init(&mg_, comm_id, world, rank, total, shard_mode), "qloco_mgpu_init");
}

ConvexMpcBatch::~ConvexMpcBatch() {
  if (mg_) qloco_mgpu_destroy(mg_);
}

void ConvexMpcBatch::check_spec() const {
  if (spec.horizon != horizon_)
    throw Error("ConvexMpcBatch: spec.horizon changed after construction (buffers sized for " +
                    std::to_string(horizon_) + ")", QLOCO_ERR_ARG);
  if (spec.warm_start != warm_mode_)
    throw Error("ConvexMpcBatch: spec.warm_start changed after construction", QLOCO_ERR_ARG);
}

void ConvexMpcBatch::reset() {
  if (!d_rec_) return;
  hip_ok(hipMemsetAsync(d_rec_, 0,
                        sizeof(float) * (size_t)batch_ * QLOCO_SRBD_PERSIST_LEN(horizon_),
                        (hipStream_t)arena_.stream()),
         "hipMemsetAsync");
}

void ConvexMpcBatch::solve_device(const float *x0, const float *x_ref, const float *feet,
                                  const uint8_t *contacts, float *u0, int32_t *st, int32_t *it) {
  check_spec();
  if (mg_)
    throw Error("ConvexMpcBatch::solve_device: a multi-GPU object solves through compute_grf "
                "(or qloco_mgpu_solve directly)", QLOCO_ERR_ARG);
  const int32_t legs = 4 * horizon_;  // constant contacts over the horizon: 4N worst case
  abi_ok(qloco_srbd_solve_model(&spec, batch_, x0, x_ref, feet, contacts, u0, nullptr, st, it,
                                nullptr, nullptr, d_rec_, legs, nullptr,
                                model_.get(), arena_.stream()),
         "qloco_srbd_solve_model");
}

void ConvexMpcBatch::compute_grf(const A1MpcState *s, double *forces) {
  check_spec();
  const size_t B = batch_, N = horizon_;
  const double dt = spec.dt;
  std::vector<float> x0(B * 13), xr(B * 13 * N), feet(B * 12);
  std::vector<uint8_t> ct(B * 4);
  int maxlegs = 0;
  for (size_t b = 0; b < B; ++b) {
    const A1MpcState &st = s[b];
    float *X = &x0[b * 13];  // mpc_states (:459-463)
    for (int k = 0; k < 3; ++k) {
      X[k] = (float)st.root_euler[k];
      X[3 + k] = (float)st.root_pos[k];
      X[6 + k] = (float)st.root_ang_vel[k];
      X[9 + k] = (float)st.root_lin_vel[k];
    }
    X[12] = -9.8f;
    // root_lin_vel_d_world = root_rot_mat * root_lin_vel_d (:479), before the
    // yaw overwrite of root_rot_mat (:502-510, done inside the kernel)
    double vw[3];
    for (int r = 0; r < 3; ++r)
      vw[r] = st.root_rot_mat[0 * 3 + r] * st.root_lin_vel_d[0] +
              st.root_rot_mat[1 * 3 + r] * st.root_lin_vel_d[1] +
              st.root_rot_mat[2 * 3 + r] * st.root_lin_vel_d[2];
    for (size_t i = 0; i < N; ++i) {  // mpc_states_d (:480-497)
      float *R = &xr[b * 13 * N + 13 * i];
      const double k = dt * (double)(i + 1);
      R[0] = (float)st.root_euler_d[0];
      R[1] = (float)st.root_euler_d[1];
      R[2] = (float)(st.root_euler[2] + st.root_ang_vel_d[2] * k);
      R[3] = (float)(st.root_pos[0] + vw[0] * k);
      R[4] = (float)(st.root_pos[1] + vw[1] * k);
      R[5] = (float)st.root_pos_d[2];
      R[6] = (float)st.root_ang_vel_d[0];
      R[7] = (float)st.root_ang_vel_d[1];
      R[8] = (float)st.root_ang_vel_d[2];
      R[9] = (float)vw[0];
      R[10] = (float)vw[1];
      R[11] = 0.0f;
      R[12] = -9.8f;
    }
    int legs = 0;
    for (int l = 0; l < 4; ++l) {
      for (int c = 0; c < 3; ++c) feet[b * 12 + 3 * l + c] = (float)st.foot_pos_abs[3 * l + c];
      ct[b * 4 + l] = st.contacts[l] ? 1 : 0;
      legs += st.contacts[l] ? 1 : 0;
    }
    if (legs * (int)N > maxlegs) maxlegs = legs * (int)N;
  }
  arena_.upload(d_x0_, x0.data(), sizeof(float) * B * 13);
  arena_.upload(d_xr_, xr.data(), sizeof(float) * B * 13 * N);
  arena_.upload(d_feet_, feet.data(), sizeof(float) * B * 12);
  arena_.upload(d_ct_, ct.data(), B * 4);
  if (mg_) {  // this rank's shard, then one all-gather of every robot's u0
    abi_ok(qloco_mgpu_solve_model(mg_, &spec, d_x0_, d_xr_, d_feet_, d_ct_, d_rec_, d_u0_all_,
                                  d_st_all_, d_it_all_, maxlegs, model_.get(), arena_.stream()),
           "qloco_mgpu_solve_model");
    const size_t T = (size_t)total_;
    std::vector<float> ua(T * 12);
    std::vector<int32_t> sa(T), ia(T);
    arena_.download(ua.data(), d_u0_all_, sizeof(float) * T * 12);
    arena_.download(sa.data(), d_st_all_, sizeof(int32_t) * T);
    arena_.download(ia.data(), d_it_all_, sizeof(int32_t) * T);
    arena_.sync();
    for (size_t g = 0; g < T; ++g)
      for (int l = 0; l < 4; ++l) {
        const float *f = &ua[g * 12 + 3 * l];
        if (std::isnan(f[0]) || std::isnan(f[1]) || std::isnan(f[2])) continue;  // :597 guard
        for (int c = 0; c < 3; ++c) all_forces_[g * 12 + 3 * l + c] = f[c];
      }
    for (size_t b = 0; b < B; ++b) {
      const size_t g = (size_t)(shard_first + (int64_t)b * shard_stride);
      status[b] = sa[g];
      iters[b] = ia[g];
      for (int l = 0; l < 4; ++l) {
        const float *f = &ua[g * 12 + 3 * l];
        if (std::isnan(f[0]) || std::isnan(f[1]) || std::isnan(f[2])) continue;
        for (int c = 0; c < 3; ++c) forces[b * 12 + 3 * l + c] = f[c];
      }
    }
    return;
  }
  abi_ok(qloco_srbd_solve_model(&spec, batch_, d_x0_, d_xr_, d_feet_, d_ct_, d_u0_, nullptr, d_st_,
                                d_it_, nullptr, nullptr, d_rec_, maxlegs, nullptr,
                                model_.get(), arena_.stream()),
         "qloco_srbd_solve_model");
  std::vector<float> u0(B * 12);
  arena_.download(u0.data(), d_u0_, sizeof(float) * B * 12);
  arena_.download(status.data(), d_st_, sizeof(int32_t) * B);
  arena_.download(iters.data(), d_it_, sizeof(int32_t) * B);
  arena_.sync();
  for (size_t b = 0; b < B; ++b)
    for (int l = 0; l < 4; ++l) {
      const float *f = &u0[b * 12 + 3 * l];
      if (std::isnan(f[0]) || std::isnan(f[1]) || std::isnan(f[2])) continue;  // :597 guard
      for (int c = 0; c < 3; ++c) forces[b * 12 + 3 * l + c] = f[c];
    }
}


// ---------------------------------------------------------------- A1QpBatch
A1QpBatch::A1QpBatch(int batch, const qloco_a1_params *p)
    : batch_(positive_batch(batch, "A1QpBatch")) {
  if (p) params = *p;
  else qloco_a1_params_default(&params);
  abi_ok(qloco_a1_params_check(&params), "A1QpBatch");  // the rule of include/qloco.h section 9
  const size_t B = batch;
  d_state_ = dalloc<double>(arena_, B * QLOCO_A1_STATE_LEN);
  d_forces_ = dalloc<double>(arena_, B * 12);
  d_ct_ = dalloc<uint8_t>(arena_, B * 4);
  d_st_ = dalloc<int32_t>(arena_, B);
  d_it_ = dalloc<int32_t>(arena_, B);
  status.assign(B, 0);
  iters.assign(B, 0);
}

void A1QpBatch::compute_grf(const A1QpState *s, double *forces) {
  const size_t B = batch_;
  std::vector<double> st(B * QLOCO_A1_STATE_LEN);
  std::vector<uint8_t> ct(B * 4);
  for (size_t b = 0; b < B; ++b) {  // the record layout of include/qloco.h section 9
    double *r = &st[b * QLOCO_A1_STATE_LEN];
    const double *src[8] = {s[b].root_pos,     s[b].root_pos_d,     s[b].root_euler,
                            s[b].root_euler_d, s[b].root_lin_vel,   s[b].root_lin_vel_d,
                            s[b].root_ang_vel, s[b].root_ang_vel_d};
    for (int f = 0; f < 8; ++f)
      for (int k = 0; k < 3; ++k) r[3 * f + k] = src[f][k];
    for (int k = 0; k < 9; ++k) {
      r[24 + k] = s[b].root_rot_mat[k];
      r[33 + k] = s[b].root_rot_mat_z[k];
    }
    for (int k = 0; k < 12; ++k) r[42 + k] = s[b].foot_pos_abs[k];
    for (int l = 0; l < 4; ++l) ct[b * 4 + l] = s[b].contacts[l] ? 1 : 0;
  }
  arena_.upload(d_state_, st.data(), sizeof(double) * st.size());
  arena_.upload(d_ct_, ct.data(), ct.size());
  abi_ok(qloco_a1_qp_solve_body(&params, batch_, d_state_, d_ct_, d_forces_, nullptr, d_st_, d_it_,
                                nullptr, nullptr, body_.get(), arena_.stream()),
         "qloco_a1_qp_solve_body");
  arena_.download(forces, d_forces_, sizeof(double) * B * 12);
  arena_.download(status.data(), d_st_, sizeof(int32_t) * B);
  arena_.download(iters.data(), d_it_, sizeof(int32_t) * B);
  arena_.sync();
}


// ---------------------------------------------------------------- A1BasicEKFBatch
// device staging, doubles per robot: dt 1 | root_rot_mat 9 | imu_acc 3 |
// imu_ang_vel 3 | foot_pos_rel 12 | foot_vel_rel 12 | foot_force 4 (= 44,
// field-major); outputs root_pos 3 | root_lin_vel 3, then x 18 | P 324
A1BasicEKFBatch::A1BasicEKFBatch(int batch, const qloco_a1_ekf_params *p)
    : batch_(positive_batch(batch, "A1BasicEKFBatch")) {
  if (p) params = *p;
  else qloco_a1_ekf_params_default(&params);
  const size_t B = batch;
  const int64_t ws = qloco_a1_ekf_workspace_bytes(batch);
  if (ws < 0) throw Error("qloco_a1_ekf_workspace_bytes", QLOCO_ERR_ARG);
  d_ws_ = arena_.alloc((size_t)ws);
  d_in_ = dalloc<double>(arena_, B * 44);
  d_out_ = dalloc<double>(arena_, B * (6 + 18 + 324));
  d_mode_ = dalloc<int32_t>(arena_, B);
  d_ct_ = dalloc<uint8_t>(arena_, B * 4);
}

A1BasicEKFBatch::A1BasicEKFBatch(int batch, bool assume_flat_ground)
    : A1BasicEKFBatch(batch, nullptr) {
  params.assume_flat_ground = assume_flat_ground ? 1 : 0;
}

void A1BasicEKFBatch::stage(const A1EstState *s, double dt) {
  const size_t B = batch_;
  std::vector<double> in(B * 44);
  std::vector<int32_t> mode(B);
  double *pdt = in.data(), *rot = pdt + B, *acc = rot + 9 * B, *om = acc + 3 * B,
         *fk = om + 3 * B, *fv = fk + 12 * B, *ff = fv + 12 * B;
  for (size_t b = 0; b < B; ++b) {
    pdt[b] = dt;
    mode[b] = s[b].movement_mode;
    for (int k = 0; k < 9; ++k) rot[9 * b + k] = s[b].root_rot_mat[k];
    for (int k = 0; k < 3; ++k) {
      acc[3 * b + k] = s[b].imu_acc[k];
      om[3 * b + k] = s[b].imu_ang_vel[k];
    }
    for (int k = 0; k < 12; ++k) {
      fk[12 * b + k] = s[b].foot_pos_rel[k];
      fv[12 * b + k] = s[b].foot_vel_rel[k];
    }
    for (int k = 0; k < 4; ++k) ff[4 * b + k] = s[b].foot_force[k];
  }
  arena_.upload(d_in_, in.data(), sizeof(double) * in.size());
  arena_.upload(d_mode_, mode.data(), sizeof(int32_t) * B);
  arena_.sync();  // the host vectors go out of scope
}

void A1BasicEKFBatch::init_state(const A1EstState *s) {
  if (!s) throw Error("A1BasicEKFBatch::init_state: null states", QLOCO_ERR_ARG);
  const size_t B = batch_;
  stage(s, 0.0);
  abi_ok(qloco_a1_ekf_init(&params, batch_, d_ws_, d_in_ + B, d_in_ + 16 * B, arena_.stream()),
         "qloco_a1_ekf_init");
  arena_.sync();
  filter_initialized_ = true;
}

void A1BasicEKFBatch::update_estimation(A1EstState *s, double dt) {
  if (!s) throw Error("A1BasicEKFBatch::update_estimation: null states", QLOCO_ERR_ARG);
  const size_t B = batch_;
  stage(s, dt);
  double *in = d_in_;
  abi_ok(qloco_a1_ekf_update(&params, batch_, d_ws_, in, d_mode_, in + B, in + 10 * B, in + 13 * B,
                             in + 16 * B, in + 28 * B, in + 40 * B, d_out_, d_out_ + 3 * B, d_ct_,
                             arena_.stream()),
         "qloco_a1_ekf_update");
  std::vector<double> out(B * 6);
  std::vector<uint8_t> ct(B * 4);
  arena_.download(out.data(), d_out_, sizeof(double) * B * 6);
  arena_.download(ct.data(), d_ct_, B * 4);
  arena_.sync();
  for (size_t b = 0; b < B; ++b) {  // A1BasicEKF.cpp:151-163
    for (int l = 0; l < 4; ++l) s[b].estimated_contacts[l] = ct[4 * b + l] != 0;
    for (int k = 0; k < 3; ++k) {
      s[b].estimated_root_pos[k] = s[b].root_pos[k] = out[3 * b + k];
      s[b].estimated_root_vel[k] = s[b].root_lin_vel[k] = out[3 * B + 3 * b + k];
    }
  }
}

void A1BasicEKFBatch::get_state(double *x, double *P) {
  if (!x || !P) throw Error("A1BasicEKFBatch::get_state: null output", QLOCO_ERR_ARG);
  const size_t B = batch_;
  double *dx = d_out_ + 6 * B, *dP = dx + 18 * B;
  abi_ok(qloco_a1_ekf_get_state(batch_, d_ws_, dx, dP, arena_.stream()), "qloco_a1_ekf_get_state");
  arena_.download(x, dx, sizeof(double) * B * 18);
  arena_.download(P, dP, sizeof(double) * B * 324);
  arena_.sync();
}


// ---------------------------------------------------------------- A1RobotControlBatch
// device staging, doubles per robot, field-major: dt 1 | root_pos 3 |
// root_lin_vel 3 | root_lin_vel_d 3 | root_rot_mat 9 | root_rot_mat_z 9 |
// foot_pos_abs 12 | foot_force 4 | root_euler_d 3 | j_foot 36 | grf 12 (= 95);
// outputs gait_counter 4 | target rel / abs / world, cur, fkin, recent 6 x 12 |
// angle 1 | torques 12 (= 89); flags contacts / plan / early 3 x 4 bytes
namespace {
constexpr size_t kCI_DT = 0, kCI_POS = 1, kCI_VEL = 4, kCI_VELD = 7, kCI_ROT = 10, kCI_ROTZ = 19,
                 kCI_FEET = 28, kCI_FORCE = 40, kCI_EUL = 44, kCI_J = 47, kCI_GRF = 83, kCI_N = 95;
constexpr size_t kCO_GC = 0, kCO_T = 4, kCO_ANG = 76, kCO_TAU = 77, kCO_N = 89;
}  // namespace

A1RobotControlBatch::A1RobotControlBatch(int batch, const qloco_a1_ctrl_params *p)
    : batch_(positive_batch(batch, "A1RobotControlBatch")) {
  if (p) params = *p;
  else qloco_a1_ctrl_params_default(&params);
  const size_t B = batch;
  const int64_t ws = qloco_a1_ctrl_workspace_bytes(batch);
  if (ws < 0) throw Error("qloco_a1_ctrl_workspace_bytes", QLOCO_ERR_ARG);
  d_ws_ = arena_.alloc((size_t)ws);
  d_in_ = dalloc<double>(arena_, B * kCI_N);
  d_out_ = dalloc<double>(arena_, B * kCO_N);
  d_rec_ = dalloc<double>(arena_, B * QLOCO_A1_CTRL_STATE);
  d_mode_ = dalloc<int32_t>(arena_, B);
  d_ct_ = dalloc<uint8_t>(arena_, B * 12);
  reset();
}

void A1RobotControlBatch::reset() {
  abi_ok(qloco_a1_ctrl_reset(&params, batch_, d_ws_, arena_.stream()), "qloco_a1_ctrl_reset");
  arena_.sync();
  staged_ = false;
}

void A1RobotControlBatch::update_plan(A1CtrlState *s, double dt) {
  if (!s) throw Error("A1RobotControlBatch::update_plan: null states", QLOCO_ERR_ARG);
  const size_t B = batch_;
  std::vector<double> in(B * kCI_FORCE + 4 * B);
  std::vector<int32_t> mode(B);
  for (size_t b = 0; b < B; ++b) {
    in[kCI_DT * B + b] = dt;
    mode[b] = s[b].movement_mode;
    for (int k = 0; k < 3; ++k) {
      in[kCI_POS * B + 3 * b + k] = s[b].root_pos[k];
      in[kCI_VEL * B + 3 * b + k] = s[b].root_lin_vel[k];
      in[kCI_VELD * B + 3 * b + k] = s[b].root_lin_vel_d[k];
    }
    for (int k = 0; k < 9; ++k) {
      in[kCI_ROT * B + 9 * b + k] = s[b].root_rot_mat[k];
      in[kCI_ROTZ * B + 9 * b + k] = s[b].root_rot_mat_z[k];
    }
    for (int k = 0; k < 12; ++k) in[kCI_FEET * B + 12 * b + k] = s[b].foot_pos_abs[k];
    for (int k = 0; k < 4; ++k) in[kCI_FORCE * B + 4 * b + k] = s[b].foot_force[k];
  }
  arena_.upload(d_in_, in.data(), sizeof(double) * in.size());
  arena_.upload(d_mode_, mode.data(), sizeof(int32_t) * B);
  arena_.sync();  // the host vectors go out of scope
  staged_ = true;
  staged_dt_ = dt;
}

void A1RobotControlBatch::generate_swing_legs_ctrl(A1CtrlState *s, double dt) {
  if (!s) throw Error("A1RobotControlBatch::generate_swing_legs_ctrl: null states", QLOCO_ERR_ARG);
  if (!staged_ || dt != staged_dt_)
    throw Error("A1RobotControlBatch::generate_swing_legs_ctrl: update_plan(states, dt) first",
                QLOCO_ERR_ARG);
  staged_ = false;
  const size_t B = batch_;
  double *in = d_in_, *o = d_out_, *t = o + kCO_T * B;
  abi_ok(qloco_a1_ctrl_plan_swing(&params, batch_, d_ws_, in, d_mode_, in + kCI_POS * B,
                                  in + kCI_VEL * B, in + kCI_VELD * B, in + kCI_ROT * B,
                                  in + kCI_ROTZ * B, in + kCI_FEET * B, in + kCI_FORCE * B, d_ct_,
                                  d_ct_ + 4 * B, d_ct_ + 8 * B, o, t, t + 12 * B, t + 24 * B,
                                  t + 36 * B, t + 48 * B, t + 60 * B, arena_.stream()),
         "qloco_a1_ctrl_plan_swing");
  std::vector<double> out(B * kCO_ANG);
  std::vector<uint8_t> ct(B * 12);
  arena_.download(out.data(), d_out_, sizeof(double) * out.size());
  arena_.download(ct.data(), d_ct_, ct.size());
  arena_.sync();
  for (size_t b = 0; b < B; ++b) {
    for (int l = 0; l < 4; ++l) {
      s[b].gait_counter[l] = out[4 * b + l];
      s[b].contacts[l] = ct[4 * b + l] != 0;
      s[b].plan_contacts[l] = ct[4 * B + 4 * b + l] != 0;
      s[b].early_contacts[l] = ct[8 * B + 4 * b + l] != 0;
    }
    double *dst[6] = {s[b].foot_pos_target_rel, s[b].foot_pos_target_abs, s[b].foot_pos_target_world,
                      s[b].foot_pos_cur,        s[b].foot_forces_kin,     s[b].foot_pos_recent_contact};
    for (int f = 0; f < 6; ++f)
      for (int k = 0; k < 12; ++k) dst[f][k] = out[(kCO_T + 12 * f) * B + 12 * b + k];
    for (int k = 0; k < 12; ++k) s[b].joint_torques[k] = 0.0;  // :210
  }
}

void A1RobotControlBatch::compute_terrain_pitch(A1CtrlState *s) {
  if (!s) throw Error("A1RobotControlBatch::compute_terrain_pitch: null states", QLOCO_ERR_ARG);
  const size_t B = batch_;
  std::vector<double> in(6 * B);
  for (size_t b = 0; b < B; ++b)
    for (int k = 0; k < 3; ++k) {
      in[3 * b + k] = s[b].root_pos[k];
      in[3 * B + 3 * b + k] = s[b].root_euler_d[k];
    }
  double *pos = d_in_ + kCI_POS * B, *eul = d_in_ + kCI_EUL * B, *ang = d_out_ + kCO_ANG * B;
  arena_.upload(pos, in.data(), sizeof(double) * 3 * B);
  arena_.upload(eul, in.data() + 3 * B, sizeof(double) * 3 * B);
  abi_ok(qloco_a1_ctrl_terrain(&params, batch_, d_ws_, pos, eul, ang, nullptr, arena_.stream()),
         "qloco_a1_ctrl_terrain");
  std::vector<double> out(4 * B);
  arena_.download(out.data(), eul, sizeof(double) * 3 * B);
  arena_.download(out.data() + 3 * B, ang, sizeof(double) * B);
  arena_.sync();
  for (size_t b = 0; b < B; ++b) {
    s[b].root_euler_d[1] = out[3 * b + 1];
    s[b].terrain_pitch_angle = out[3 * B + b];
  }
}

void A1RobotControlBatch::compute_joint_torques(A1CtrlState *s) {
  if (!s) throw Error("A1RobotControlBatch::compute_joint_torques: null states", QLOCO_ERR_ARG);
  const size_t B = batch_;
  std::vector<double> in(48 * B);
  for (size_t b = 0; b < B; ++b) {
    for (int k = 0; k < 36; ++k) in[36 * b + k] = s[b].j_foot[k];
    for (int k = 0; k < 12; ++k) in[36 * B + 12 * b + k] = s[b].foot_forces_grf[k];
  }
  double *J = d_in_ + kCI_J * B, *grf = d_in_ + kCI_GRF * B, *tau = d_out_ + kCO_TAU * B;
  arena_.upload(J, in.data(), sizeof(double) * 48 * B);  // j_foot and grf are adjacent
  abi_ok(qloco_a1_ctrl_joint_torques(&params, batch_, d_ws_, J, grf, tau, arena_.stream()),
         "qloco_a1_ctrl_joint_torques");
  std::vector<double> out(12 * B);
  arena_.download(out.data(), tau, sizeof(double) * 12 * B);
  arena_.sync();
  for (size_t b = 0; b < B; ++b)
    for (int k = 0; k < 12; ++k) s[b].joint_torques[k] = out[12 * b + k];
}

void A1RobotControlBatch::get_state(double *state) {
  if (!state) throw Error("A1RobotControlBatch::get_state: null output", QLOCO_ERR_ARG);
  abi_ok(qloco_a1_ctrl_get_state(batch_, d_ws_, d_rec_, arena_.stream()), "qloco_a1_ctrl_get_state");
  arena_.download(state, d_rec_, sizeof(double) * (size_t)batch_ * QLOCO_A1_CTRL_STATE);
  arena_.sync();
}


// ------------------------------------------------------------------------
// NLPStepTimingBatch -> qloco_nlp_*
namespace {
// device input block, per robot: est[6] | rfoot[2] | lfoot[2]; output block:
// vari[4] | step[3] | com[18]; int block: sched[4] | status[1]
constexpr size_t kNI_EST = 0, kNI_RF = 6, kNI_LF = 8, kNI_N = 10;
constexpr size_t kNO_VARI = 0, kNO_STEP = 4, kNO_COM = 7, kNO_N = 25;
}  // namespace

NLPStepTimingBatch::NLPStepTimingBatch(int batch, double stepwidth, double steplength, double stepheight,
                                       const qloco_nlp_params *p)
    : batch_(positive_batch(batch, "NLPStepTimingBatch")), stepheight_(stepheight) {
  if (p) params = *p;
  else qloco_nlp_params_default(&params);
  const size_t B = batch;
  const int64_t ws = qloco_nlp_workspace_bytes(batch);
  if (ws < 0) throw Error("qloco_nlp_workspace_bytes", QLOCO_ERR_ARG);
  d_ws_ = arena_.alloc((size_t)ws);
  d_in_ = dalloc<double>(arena_, B * kNI_N);
  d_out_ = dalloc<double>(arena_, B * kNO_N);
  d_rec_ = dalloc<double>(arena_, B * QLOCO_NLP_STATE);
  d_i_ = dalloc<int32_t>(arena_, B);
  d_int_ = dalloc<int32_t>(arena_, B * 5);
  status_.assign(B, QLOCO_OK);
  std::vector<double> in(2 * B);
  for (size_t b = 0; b < B; ++b) {
    in[b] = steplength;
    in[B + b] = stepwidth;
  }
  arena_.upload(d_in_, in.data(), sizeof(double) * in.size());
  abi_ok(qloco_nlp_init(&params, batch_, d_ws_, d_in_, d_in_ + B, nullptr, arena_.stream()), "qloco_nlp_init");
  arena_.sync();
}

void NLPStepTimingBatch::step_timing_opti_loop(int i, const double *est, const double *rfoot, const double *lfoot,
                                               double /*lamda*/, bool /*stopwalking*/, double *com_traj) {
  if (!est || !rfoot || !lfoot || !com_traj)
    throw Error("NLPStepTimingBatch::step_timing_opti_loop: null argument", QLOCO_ERR_ARG);
  const size_t B = batch_;
  std::vector<double> in(B * kNI_N);
  std::vector<int32_t> ti(B, i);
  for (size_t b = 0; b < B; ++b) {
    for (int k = 0; k < 6; ++k) in[kNI_EST * B + 6 * b + k] = est[18 * b + k];
    for (int k = 0; k < 2; ++k) {
      in[kNI_RF * B + 2 * b + k] = rfoot[3 * b + k];
      in[kNI_LF * B + 2 * b + k] = lfoot[3 * b + k];
    }
  }
  arena_.upload(d_in_, in.data(), sizeof(double) * in.size());
  arena_.upload(d_i_, ti.data(), sizeof(int32_t) * B);
  abi_ok(qloco_nlp_step_timing(&params, batch_, d_ws_, d_i_, d_in_ + kNI_EST * B, d_in_ + kNI_RF * B,
                               d_in_ + kNI_LF * B, d_out_ + kNO_VARI * B, d_int_, d_out_ + kNO_STEP * B,
                               d_out_ + kNO_COM * B, nullptr, nullptr, d_int_ + 4 * B, arena_.stream()),
         "qloco_nlp_step_timing");
  abi_ok(qloco_nlp_get_state(batch_, d_ws_, d_rec_, arena_.stream()), "qloco_nlp_get_state");
  std::vector<double> out(B * kNO_N), rec(B * QLOCO_NLP_STATE);
  std::vector<int32_t> ints(B * 5);
  arena_.download(out.data(), d_out_, sizeof(double) * out.size());
  arena_.download(rec.data(), d_rec_, sizeof(double) * rec.size());
  arena_.download(ints.data(), d_int_, sizeof(int32_t) * ints.size());
  arena_.sync();
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (size_t b = 0; b < B; ++b) {
    double *c = com_traj + kComTraj * b;
    for (int k = 0; k < kComTraj; ++k) c[k] = nan;  // 2, 5, 8, 9..20, 23, 26 stay NaN
    status_[b] = ints[4 * B + b];
    if (status_[b] != QLOCO_OK && status_[b] != QLOCO_NAN) continue;
    const double *com = &out[kNO_COM * B + 18 * b], *step = &out[kNO_STEP * B + 3 * b];
    const double *fx = &rec[QLOCO_NLP_STATE * b + 135], *fy = &rec[QLOCO_NLP_STATE * b + 162];
    const int period = ints[4 * b + 0], bjxx = ints[4 * b + 2];
    c[0] = com[0];  // :1048-1056
    c[1] = com[1];
    c[3] = com[2];
    c[4] = com[3];
    c[6] = com[4];
    c[7] = com[5];
    c[21] = com[6 + 4];  // :1072-1077
    c[22] = com[6 + 5];
    c[24] = com[12 + 4];
    c[25] = com[12 + 5];
    c[27] = bjxx;  // :1079-1090
    if (bjxx >= 0 && bjxx + 1 < QLOCO_NLP_STEPS) {
      c[28] = fx[bjxx];
      c[29] = fx[bjxx + 1];
      c[30] = fy[bjxx];
      c[31] = fy[bjxx + 1];
      // _footz_ref(k) = k * stepheight accumulated as the reference does (:180)
      double z = 0.0, z0 = 0.0, z1 = 0.0;
      for (int k = 0; k <= bjxx + 1; ++k) {
        if (k == bjxx) z0 = z;
        if (k == bjxx + 1) z1 = z;
        z = z + stepheight_;
      }
      c[32] = z0;
      c[33] = z1;
    }
    c[34] = period - 1;
    c[35] = step[0];
    c[36] = step[1];
    c[37] = step[2];
  }
}

std::array<double, 38> NLPStepTimingBatch::step_timing_opti_loop(int i, const double estimated_state[18],
                                                                 const double Rfoot[3], const double Lfoot[3],
                                                                 double lamda, bool stopwalking) {
  if (batch_ != 1) throw Error("NLPStepTimingBatch: the single-robot call needs batch 1", QLOCO_ERR_ARG);
  std::array<double, 38> r;
  step_timing_opti_loop(i, estimated_state, Rfoot, Lfoot, lamda, stopwalking, r.data());
  return r;
}

void NLPStepTimingBatch::get_state(double *state) {
  if (!state) throw Error("NLPStepTimingBatch::get_state: null output", QLOCO_ERR_ARG);
  abi_ok(qloco_nlp_get_state(batch_, d_ws_, d_rec_, arena_.stream()), "qloco_nlp_get_state");
  arena_.download(state, d_rec_, sizeof(double) * (size_t)batch_ * QLOCO_NLP_STATE);
  arena_.sync();
}

void NLPStepTimingBatch::set_state(const double *state) {
  if (!state) throw Error("NLPStepTimingBatch::set_state: null input", QLOCO_ERR_ARG);
  arena_.upload(d_rec_, state, sizeof(double) * (size_t)batch_ * QLOCO_NLP_STATE);
  abi_ok(qloco_nlp_set_state(batch_, d_ws_, d_rec_, arena_.stream()), "qloco_nlp_set_state");
  arena_.sync();
}

// ------------------------------------------------------------------------
// NLPClassBatch -> qloco_nlp_tick
namespace {
// device input block, per robot: est[6] | rfoot[2] | lfoot[2] | stepheight[1];
// output block: com_traj[38] | rlfoot[18] | vari[4]; int block: t_int | stop |
// right_support | status
constexpr size_t kTI_N = 11, kTO_CT = 0, kTO_RL = 38, kTO_VARI = 56, kTO_N = 60;
}  // namespace

NLPClassBatch::NLPClassBatch(int batch, double stepwidth, double steplength, double stepheight,
                             const qloco_nlp_params *p, const qloco_nlp_tick_params *tp)
    : batch_(positive_batch(batch, "NLPClassBatch")) {
  if (p) params = *p;
  else qloco_nlp_params_default(&params);
  if (tp) tick_params = *tp;
  else qloco_nlp_tick_params_default(&tick_params);
  const size_t B = batch;
  const int64_t ws = qloco_nlp_workspace_bytes(batch), tws = qloco_nlp_tick_workspace_bytes(batch);
  if (ws < 0 || tws < 0) throw Error("qloco_nlp_tick_workspace_bytes", QLOCO_ERR_ARG);
  d_ws_ = arena_.alloc((size_t)ws);
  d_tws_ = arena_.alloc((size_t)tws);
  d_in_ = dalloc<double>(arena_, B * kTI_N);
  d_out_ = dalloc<double>(arena_, B * kTO_N);
  d_rec_ = dalloc<double>(arena_, B * QLOCO_NLP_STATE);
  d_trec_ = dalloc<double>(arena_, B * QLOCO_NLP_TICK_STATE);
  d_i_ = dalloc<int32_t>(arena_, 2 * B);
  d_int_ = dalloc<int32_t>(arena_, 2 * B);
  status_.assign(B, QLOCO_OK);
  right_support_batch.assign(B, 0);
  foot_.assign(B * kFootTraj, 0.0);
  std::vector<double> in(3 * B);
  for (size_t b = 0; b < B; ++b) {
    in[b] = steplength;
    in[B + b] = stepwidth;
    in[2 * B + b] = stepheight;
  }
  arena_.upload(d_in_, in.data(), sizeof(double) * in.size());
  abi_ok(qloco_nlp_tick_init(&params, &tick_params, batch_, d_ws_, d_tws_, d_in_, d_in_ + B, d_in_ + 2 * B,
                             arena_.stream()),
         "qloco_nlp_tick_init");
  arena_.sync();
}

void NLPClassBatch::step_timing_opti_loop(int i, const double *est, const double *rfoot, const double *lfoot,
                                          double /*lamda*/, bool stopwalking, double *com_traj) {
  if (!est || !rfoot || !lfoot || !com_traj)
    throw Error("NLPClassBatch::step_timing_opti_loop: null argument", QLOCO_ERR_ARG);
  const size_t B = batch_;
  std::vector<double> in(B * 10);
  std::vector<int32_t> ti(2 * B, i);
  for (size_t b = 0; b < B; ++b) {
    for (int k = 0; k < 6; ++k) in[6 * b + k] = est[18 * b + k];
    for (int k = 0; k < 2; ++k) {
      in[6 * B + 2 * b + k] = rfoot[3 * b + k];
      in[8 * B + 2 * b + k] = lfoot[3 * b + k];
    }
    ti[B + b] = stopwalking ? 1 : 0;
  }
  arena_.upload(d_in_, in.data(), sizeof(double) * in.size());
  arena_.upload(d_i_, ti.data(), sizeof(int32_t) * ti.size());
  abi_ok(qloco_nlp_tick(&params, &tick_params, batch_, d_ws_, d_tws_, d_i_, d_in_, d_in_ + 6 * B, d_in_ + 8 * B,
                        d_i_ + B, d_out_ + kTO_CT * B, d_out_ + kTO_RL * B, d_int_, d_out_ + kTO_VARI * B, nullptr,
                        nullptr, nullptr, nullptr, nullptr, d_int_ + B, arena_.stream()),
         "qloco_nlp_tick");
  std::vector<int32_t> ints(2 * B);
  arena_.download(com_traj, d_out_ + kTO_CT * B, sizeof(double) * B * kComTraj);
  arena_.download(foot_.data(), d_out_ + kTO_RL * B, sizeof(double) * B * kFootTraj);
  arena_.download(ints.data(), d_int_, sizeof(int32_t) * ints.size());
  arena_.sync();
  for (size_t b = 0; b < B; ++b) {
    right_support_batch[b] = ints[b];
    status_[b] = ints[B + b];
  }
  right_support = right_support_batch[0];
  last_i_ = i;
  last_stop_ = stopwalking;
  have_tick_ = true;
}

std::array<double, 38> NLPClassBatch::step_timing_opti_loop(int i, const double estimated_state[18],
                                                            const double Rfoot[3], const double Lfoot[3],
                                                            double lamda, bool stopwalking) {
  if (batch_ != 1) throw Error("NLPClassBatch: the single-robot call needs batch 1", QLOCO_ERR_ARG);
  std::array<double, 38> r;
  step_timing_opti_loop(i, estimated_state, Rfoot, Lfoot, lamda, stopwalking, r.data());
  return r;
}

void NLPClassBatch::Foot_trajectory_solve_mod2(int j_index, bool stopwalking, double *rlfoot_traj) {
  if (!rlfoot_traj) throw Error("NLPClassBatch::Foot_trajectory_solve_mod2: null output", QLOCO_ERR_ARG);
  if (!have_tick_ || j_index != last_i_ || stopwalking != last_stop_)
    throw Error("NLPClassBatch::Foot_trajectory_solve_mod2: call step_timing_opti_loop with the same index and "
                "stopwalking first",
                QLOCO_ERR_ARG);
  std::copy(foot_.begin(), foot_.end(), rlfoot_traj);
}

std::array<double, 18> NLPClassBatch::Foot_trajectory_solve_mod2(int j_index, bool stopwalking) {
  if (batch_ != 1) throw Error("NLPClassBatch: the single-robot call needs batch 1", QLOCO_ERR_ARG);
  std::array<double, 18> r;
  Foot_trajectory_solve_mod2(j_index, stopwalking, r.data());
  return r;
}

void NLPClassBatch::get_state(double *nlp_state, double *tick_state) {
  if (!nlp_state || !tick_state) throw Error("NLPClassBatch::get_state: null output", QLOCO_ERR_ARG);
  abi_ok(qloco_nlp_get_state(batch_, d_ws_, d_rec_, arena_.stream()), "qloco_nlp_get_state");
  abi_ok(qloco_nlp_tick_get_state(batch_, d_tws_, d_trec_, arena_.stream()), "qloco_nlp_tick_get_state");
  arena_.download(nlp_state, d_rec_, sizeof(double) * (size_t)batch_ * QLOCO_NLP_STATE);
  arena_.download(tick_state, d_trec_, sizeof(double) * (size_t)batch_ * QLOCO_NLP_TICK_STATE);
  arena_.sync();
}

void NLPClassBatch::set_state(const double *nlp_state, const double *tick_state) {
  if (!nlp_state || !tick_state) throw Error("NLPClassBatch::set_state: null input", QLOCO_ERR_ARG);
  arena_.upload(d_rec_, nlp_state, sizeof(double) * (size_t)batch_ * QLOCO_NLP_STATE);
  arena_.upload(d_trec_, tick_state, sizeof(double) * (size_t)batch_ * QLOCO_NLP_TICK_STATE);
  abi_ok(qloco_nlp_set_state(batch_, d_ws_, d_rec_, arena_.stream()), "qloco_nlp_set_state");
  abi_ok(qloco_nlp_tick_set_state(batch_, d_tws_, d_trec_, arena_.stream()), "qloco_nlp_tick_set_state");
  arena_.sync();
}

// ------------------------------------------------------------------------
// NLPRTControlBatch -> qloco_nlp_node_*
NLPRTControlBatch::NLPRTControlBatch(int batch, double stepheight, const qloco_nlp_params *p,
                                     const qloco_nlp_tick_params *tp, const qloco_nlp_node_params *np)
    : batch_(positive_batch(batch, "NLPRTControlBatch")) {
  if (p) params = *p;
  else qloco_nlp_params_default(&params);
  if (tp) tick_params = *tp;
  else qloco_nlp_tick_params_default(&tick_params);
  if (np) node_params = *np;
  else qloco_nlp_node_params_default(&node_params);
  const size_t B = batch;
  const int64_t ws = qloco_nlp_workspace_bytes(batch), tws = qloco_nlp_tick_workspace_bytes(batch);
  const int64_t nws = qloco_nlp_node_workspace_bytes(batch);
  if (ws < 0 || tws < 0 || nws < 0) throw Error("qloco_nlp_node_workspace_bytes", QLOCO_ERR_ARG);
  d_ws_ = arena_.alloc((size_t)ws);
  d_tws_ = arena_.alloc((size_t)tws);
  d_nws_ = arena_.alloc((size_t)nws);
  d_msg_ = dalloc<double>(arena_, B * QLOCO_NRT_MSG_LEN);
  d_row_ = dalloc<double>(arena_, B * kRow);
  d_rec_ = dalloc<double>(arena_, B * QLOCO_NLP_STATE);
  d_trec_ = dalloc<double>(arena_, B * QLOCO_NLP_TICK_STATE);
  d_nrec_ = dalloc<double>(arena_, B * QLOCO_NLP_NODE_STATE);
  d_int_ = dalloc<int32_t>(arena_, B * (QLOCO_NLP_NODE_SCHED_LEN + 1));
  // stepwidthinput = 2 HALF_HIP_WIDTH, steplengthinput = 0.075 ("go1", NLPRTControlClass.cpp:63-71)
  std::vector<double> in(3 * B);
  for (size_t b = 0; b < B; ++b) {
    in[b] = 0.075;
    in[B + b] = params.half_hip_width * 2;
    in[2 * B + b] = stepheight;
  }
  arena_.upload(d_rec_, in.data(), sizeof(double) * in.size());
  abi_ok(qloco_nlp_node_init(&params, &tick_params, &node_params, batch_, d_ws_, d_tws_, d_nws_, d_rec_, d_rec_ + B,
                             d_rec_ + 2 * B, arena_.stream()),
         "qloco_nlp_node_init");
  arena_.sync();
}

void NLPRTControlBatch::tick(const double *d_nrt_msg, double *d_gait_msg, int32_t *d_sched, int32_t *d_status) {
  abi_ok(qloco_nlp_node_tick(&params, &tick_params, &node_params, batch_, d_ws_, d_tws_, d_nws_, d_nrt_msg,
                             d_gait_msg, d_sched, d_status, arena_.stream()),
         "qloco_nlp_node_tick");
}

std::array<double, 100> NLPRTControlBatch::WalkingReactStepping(int walkdtime, bool start_mpc,
                                                                const double /*estimated_state*/[18],
                                                                const double Rfoot[3], const double Lfoot[3]) {
  if (batch_ != 1) throw Error("NLPRTControlBatch: the single-robot call needs batch 1", QLOCO_ERR_ARG);
  if (!Rfoot || !Lfoot) throw Error("NLPRTControlBatch::WalkingReactStepping: null argument", QLOCO_ERR_ARG);
  double msg[QLOCO_NRT_MSG_LEN] = {0};
  if (start_mpc && walkdtime == count_ + 1) {
    msg[0] = 1.0;  // the loop's own step: the device advances count and latch
  } else if (!(start_mpc == latch_ && walkdtime == count_)) {
    // any other caller: write the two members the loop would hold
    std::vector<double> rec(QLOCO_NLP_NODE_STATE);
    abi_ok(qloco_nlp_node_get_state(1, d_nws_, d_nrec_, arena_.stream()), "qloco_nlp_node_get_state");
    arena_.download(rec.data(), d_nrec_, sizeof(double) * rec.size());
    arena_.sync();
    rec[0] = walkdtime;
    rec[1] = start_mpc ? 1.0 : 0.0;
    arena_.upload(d_nrec_, rec.data(), sizeof(double) * rec.size());
    abi_ok(qloco_nlp_node_set_state(1, d_nws_, d_nrec_, arena_.stream()), "qloco_nlp_node_set_state");
  }
  count_ = walkdtime;
  latch_ = start_mpc;
  for (int k = 0; k < 3; ++k) {
    msg[19 + k] = Lfoot[k];
    msg[22 + k] = Rfoot[k];
  }
  arena_.upload(d_msg_, msg, sizeof(msg));
  tick(d_msg_, d_row_, d_int_, d_int_ + QLOCO_NLP_NODE_SCHED_LEN);
  std::array<double, 100> row;
  int32_t ints[QLOCO_NLP_NODE_SCHED_LEN + 1];
  arena_.download(row.data(), d_row_, sizeof(double) * kRow);
  arena_.download(ints, d_int_, sizeof(ints));
  arena_.sync();
  for (int k = 0; k < QLOCO_NLP_NODE_SCHED_LEN; ++k) sched[k] = ints[k];
  status = ints[QLOCO_NLP_NODE_SCHED_LEN];
  mpc_stop = row[97];
  right_support = (int)row[99];
  return row;
}

void NLPRTControlBatch::get_state(double *nlp_state, double *tick_state, double *node_state) {
  if (!nlp_state || !tick_state || !node_state) throw Error("NLPRTControlBatch::get_state: null output", QLOCO_ERR_ARG);
  const size_t B = batch_;
  abi_ok(qloco_nlp_get_state(batch_, d_ws_, d_rec_, arena_.stream()), "qloco_nlp_get_state");
  abi_ok(qloco_nlp_tick_get_state(batch_, d_tws_, d_trec_, arena_.stream()), "qloco_nlp_tick_get_state");
  abi_ok(qloco_nlp_node_get_state(batch_, d_nws_, d_nrec_, arena_.stream()), "qloco_nlp_node_get_state");
  arena_.download(nlp_state, d_rec_, sizeof(double) * B * QLOCO_NLP_STATE);
  arena_.download(tick_state, d_trec_, sizeof(double) * B * QLOCO_NLP_TICK_STATE);
  arena_.download(node_state, d_nrec_, sizeof(double) * B * QLOCO_NLP_NODE_STATE);
  arena_.sync();
}

void NLPRTControlBatch::set_state(const double *nlp_state, const double *tick_state, const double *node_state) {
  if (!nlp_state || !tick_state || !node_state) throw Error("NLPRTControlBatch::set_state: null input", QLOCO_ERR_ARG);
  const size_t B = batch_;
  arena_.upload(d_rec_, nlp_state, sizeof(double) * B * QLOCO_NLP_STATE);
  arena_.upload(d_trec_, tick_state, sizeof(double) * B * QLOCO_NLP_TICK_STATE);
  arena_.upload(d_nrec_, node_state, sizeof(double) * B * QLOCO_NLP_NODE_STATE);
  abi_ok(qloco_nlp_set_state(batch_, d_ws_, d_rec_, arena_.stream()), "qloco_nlp_set_state");
  abi_ok(qloco_nlp_tick_set_state(batch_, d_tws_, d_trec_, arena_.stream()), "qloco_nlp_tick_set_state");
  abi_ok(qloco_nlp_node_set_state(batch_, d_nws_, d_nrec_, arena_.stream()), "qloco_nlp_node_set_state");
  arena_.sync();
  if (batch_ == 1) {
    count_ = (int)node_state[0];
    latch_ = node_state[1] != 0.0;
  }
}

// ------------------------------------------------------------------------
// Kinematicclass -> qloco_leg_fk / qloco_leg_ik
Kinematicclass::Kinematicclass(int max_legs) : cap_(0) {
  if (max_legs < 1) throw Error("Kinematicclass: max_legs < 1", QLOCO_ERR_ARG);
  ensure(max_legs);
}

void Kinematicclass::ensure(int n) {
  if (n <= cap_) return;
  const size_t N = n;
  d_a_ = dalloc<double>(arena_, N * 3);
  d_b_ = dalloc<double>(arena_, N * 3);
  d_p_ = dalloc<double>(arena_, N * 3);
  d_r_ = dalloc<double>(arena_, N * 3);
  d_q_ = dalloc<double>(arena_, N * 3);
  d_pos_ = dalloc<double>(arena_, N * 3);
  d_jac_ = dalloc<double>(arena_, N * 9);
  d_leg_ = dalloc<int32_t>(arena_, N);
  d_upd_ = dalloc<int32_t>(arena_, N);
  cap_ = n;
}

void Kinematicclass::forward_batch(int n, const double *q, const int32_t *leg,
                                   const double *body_p, const double *body_r, double *pos,
                                   double *jac) {
  if (n < 0 || (n > 0 && (!q || !leg || !pos)) || ((body_p == nullptr) != (body_r == nullptr)))
    throw Error("Kinematicclass::forward_batch: bad arguments", QLOCO_ERR_ARG);
  if (n == 0) return;
  ensure(n);
  const size_t N = n;
  const bool g = body_p != nullptr;
  arena_.upload(d_q_, q, sizeof(double) * N * 3);
  arena_.upload(d_leg_, leg, sizeof(int32_t) * N);
  if (g) {
    arena_.upload(d_p_, body_p, sizeof(double) * N * 3);
    arena_.upload(d_r_, body_r, sizeof(double) * N * 3);
  }
  abi_ok(qloco_leg_fk(n, d_q_, d_leg_, g ? d_p_ : nullptr, g ? d_r_ : nullptr, d_pos_,
                      jac ? d_jac_ : nullptr, arena_.stream()),
         "qloco_leg_fk");
  arena_.download(pos, d_pos_, sizeof(double) * N * 3);
  if (jac) arena_.download(jac, d_jac_, sizeof(double) * N * 9);
  arena_.sync();
}

void Kinematicclass::inverse_batch(int n, const double *pos_des, const double *q_ini,
                                   const int32_t *leg, const double *body_p,
                                   const double *body_r, double *q_out, double *pos_out,
                                   double *jac, int32_t *updates) {
  if (n < 0 || (n > 0 && (!pos_des || !q_ini || !leg || !q_out)) ||
      ((body_p == nullptr) != (body_r == nullptr)))
    throw Error("Kinematicclass::inverse_batch: bad arguments", QLOCO_ERR_ARG);
  if (n == 0) return;
  ensure(n);
  const size_t N = n;
  const bool g = body_p != nullptr;
  arena_.upload(d_a_, pos_des, sizeof(double) * N * 3);
  arena_.upload(d_b_, q_ini, sizeof(double) * N * 3);
  arena_.upload(d_leg_, leg, sizeof(int32_t) * N);
  if (g) {
    arena_.upload(d_p_, body_p, sizeof(double) * N * 3);
    arena_.upload(d_r_, body_r, sizeof(double) * N * 3);
  }
  abi_ok(qloco_leg_ik(n, d_a_, d_b_, d_leg_, g ? d_p_ : nullptr, g ? d_r_ : nullptr, d_q_, d_pos_,
                      d_jac_, d_upd_, arena_.stream()),
         "qloco_leg_ik");
  arena_.download(q_out, d_q_, sizeof(double) * N * 3);
  if (pos_out) arena_.download(pos_out, d_pos_, sizeof(double) * N * 3);
  if (jac) arena_.download(jac, d_jac_, sizeof(double) * N * 9);
  if (updates) arena_.download(updates, d_upd_, sizeof(int32_t) * N);
  arena_.sync();
}

std::array<double, 3> Kinematicclass::Forward_kinematics(const double q_joint[3], int feet_flag) {
  std::array<double, 3> p{};
  const int32_t leg = feet_flag;
  forward_batch(1, q_joint, &leg, nullptr, nullptr, p.data(), Jacobian_kin.data());
  return p;
}

std::array<double, 3> Kinematicclass::Forward_kinematics_g(const double body_P[3],
                                                           const double body_R[3],
                                                           const double q_joint[3],
                                                           int feet_flag) {
  std::array<double, 3> p{};
  const int32_t leg = feet_flag;
  forward_batch(1, q_joint, &leg, body_P, body_R, p.data(), Jacobian_kin.data());
  return p;
}

std::array<double, 3> Kinematicclass::Inverse_kinematics(const double pos_des[3],
                                                         const double q_ini[3], int feet_flag) {
  std::array<double, 3> q{};
  const int32_t leg = feet_flag;
  int32_t upd = 0;
  inverse_batch(1, pos_des, q_ini, &leg, nullptr, nullptr, q.data(), pos_cal.data(),
                Jacobian_kin.data(), &upd);
  last_updates = upd;
  return q;
}

std::array<double, 3> Kinematicclass::Inverse_kinematics_g(const double body_P[3],
                                                           const double body_R[3],
                                                           const double pos_des[3],
                                                           const double q_ini[3],
                                                           int feet_flag) {
  std::array<double, 3> q{};
  const int32_t leg = feet_flag;
  int32_t upd = 0;
  inverse_batch(1, pos_des, q_ini, &leg, body_P, body_R, q.data(), pos_cal.data(),
                Jacobian_kin.data(), &upd);
  last_updates = upd;
  return q;
}


// ---------------------------------------------------------------- RtMpcNode
RtMpcNode::RtMpcNode(int batch) : batch_(batch) {
  if (batch < 1) throw Error("RtMpcNode: batch < 1", QLOCO_ERR_ARG);
  const size_t B = batch;
  gait_.assign(B * QLOCO_GAIT_MSG_LEN, 0.0);  // low_mpc_gait.setZero() (gait_fast.cpp:387)
  ctrl_.assign(B * QLOCO_CTRL_MSG_LEN, 0.0);
  traj.assign(B * QLOCO_TRAJ_MSG_LEN, 0.0);
  nrt.assign(B * QLOCO_NRT_MSG_LEN, 0.0);
  sched.assign(B * QLOCO_RT_SCHED_LEN, 0);
  const int64_t ws = qloco_rt_workspace_bytes(batch);
  if (ws < 0) throw Error("qloco_rt_workspace_bytes", QLOCO_ERR_ARG);
  d_ws_ = arena_.alloc((size_t)ws);
  d_gait_ = dalloc<double>(arena_, B * QLOCO_GAIT_MSG_LEN);
  d_ctrl_ = dalloc<double>(arena_, B * QLOCO_CTRL_MSG_LEN);
  d_traj_ = dalloc<double>(arena_, B * QLOCO_TRAJ_MSG_LEN);
  d_nrt_ = dalloc<double>(arena_, B * QLOCO_NRT_MSG_LEN);
  d_sched_ = dalloc<int32_t>(arena_, B * QLOCO_RT_SCHED_LEN);
  abi_ok(qloco_rt_init(batch, d_ws_, arena_.stream()), "qloco_rt_init");
  arena_.sync();
}

void RtMpcNode::nrt_gait_sub_operation(const double msg[QLOCO_GAIT_MSG_LEN], int robot) {
  if (robot < 0 || robot >= batch_) throw Error("RtMpcNode: robot out of range", QLOCO_ERR_ARG);
  std::copy(msg, msg + QLOCO_GAIT_MSG_LEN, gait_.begin() + (size_t)robot * QLOCO_GAIT_MSG_LEN);
}

void RtMpcNode::control_gait_sub_operation(const double msg[QLOCO_CTRL_MSG_LEN], int robot) {
  if (robot < 0 || robot >= batch_) throw Error("RtMpcNode: robot out of range", QLOCO_ERR_ARG);
  std::copy(msg, msg + QLOCO_CTRL_MSG_LEN, ctrl_.begin() + (size_t)robot * QLOCO_CTRL_MSG_LEN);
}

void RtMpcNode::loop_once() {
  const size_t B = batch_;
  arena_.upload(d_gait_, gait_.data(), sizeof(double) * B * QLOCO_GAIT_MSG_LEN);
  arena_.upload(d_ctrl_, ctrl_.data(), sizeof(double) * B * QLOCO_CTRL_MSG_LEN);
  abi_ok(qloco_rt_tick(batch_, d_ws_, d_gait_, d_ctrl_, d_traj_, d_nrt_, nullptr, d_sched_,
                       arena_.stream()),
         "qloco_rt_tick");
  arena_.download(traj.data(), d_traj_, sizeof(double) * B * QLOCO_TRAJ_MSG_LEN);
  arena_.download(nrt.data(), d_nrt_, sizeof(double) * B * QLOCO_NRT_MSG_LEN);
  arena_.download(sched.data(), d_sched_, sizeof(int32_t) * B * QLOCO_RT_SCHED_LEN);
  arena_.sync();
}


// ---------------------------------------------------------------- ServoForceBlock
// double inputs, per robot: coma 3, com 3, rfoot 3, lfoot 3, body_p 3, foot 12,
// y 1, Jaco 36, rel_mea 12, v_est 12 (= 88); int inputs: rs, mode, count (3);
// double outputs: F_sum 6, FLR 6, grf 12, tau 12 (= 36); int outputs: swing 4, qps, status (6)
ServoForceBlock::ServoForceBlock(int batch, const qloco_force_params *params) : batch_(batch) {
  if (batch < 1) throw Error("ServoForceBlock: batch < 1", QLOCO_ERR_ARG);
  if (params) prm_ = *params;
  else qloco_force_params_default(&prm_);
  const size_t B = batch;
  F_sum.assign(B * 6, 0.0);
  Force_L_R.assign(B * 6, 0.0);
  grf_opt.assign(B * 12, 0.0);
  Legs_torque.assign(B * 12, 0.0);
  swing.assign(B * 4, 0);
  qp_solution.assign(B, 1);
  status.assign(B, 0);
  const int64_t ws = qloco_servo_workspace_bytes(batch);
  if (ws < 0) throw Error("qloco_servo_workspace_bytes", QLOCO_ERR_ARG);
  d_ws_ = arena_.alloc((size_t)ws);
  d_in_ = dalloc<double>(arena_, B * 88);
  d_out_ = dalloc<double>(arena_, B * 36);
  d_iin_ = dalloc<int32_t>(arena_, B * 3);
  d_iout_ = dalloc<int32_t>(arena_, B * 6);
  abi_ok(qloco_servo_init(batch, d_ws_, arena_.stream()), "qloco_servo_init");
  arena_.sync();
}

void ServoForceBlock::step(const double *coma_des, const double *com_des, const double *rfoot_des,
                           const double *lfoot_des, const double *body_p_des,
                           const double *foot_des, const int32_t *right_support,
                           const int32_t *gait_mode, const double *y_offset,
                           const int32_t *count_in_rt_loop, const double *Jaco,
                           const double *foot_rel_mea, const double *v_est_rel) {
  const size_t B = batch_;
  double *in = d_in_;
  double *coma = in, *com = coma + 3 * B, *rf = com + 3 * B, *lf = rf + 3 * B, *bp = lf + 3 * B,
         *ft = bp + 3 * B, *y = ft + 12 * B, *J = y + B, *rm = J + 36 * B, *ve = rm + 12 * B;
  int32_t *rs = d_iin_, *md = rs + B, *cnt = md + B;
  arena_.upload(coma, coma_des, sizeof(double) * 3 * B);
  arena_.upload(com, com_des, sizeof(double) * 3 * B);
  arena_.upload(rf, rfoot_des, sizeof(double) * 3 * B);
  arena_.upload(lf, lfoot_des, sizeof(double) * 3 * B);
  arena_.upload(bp, body_p_des, sizeof(double) * 3 * B);
  arena_.upload(ft, foot_des, sizeof(double) * 12 * B);
  arena_.upload(y, y_offset, sizeof(double) * B);
  arena_.upload(J, Jaco, sizeof(double) * 36 * B);
  arena_.upload(rm, foot_rel_mea, sizeof(double) * 12 * B);
  arena_.upload(ve, v_est_rel, sizeof(double) * 12 * B);
  arena_.upload(rs, right_support, sizeof(int32_t) * B);
  arena_.upload(md, gait_mode, sizeof(int32_t) * B);
  arena_.upload(cnt, count_in_rt_loop, sizeof(int32_t) * B);
  double *Fs = d_out_, *Fl = Fs + 6 * B, *g = Fl + 6 * B, *tau = g + 12 * B;
  int32_t *sw = d_iout_, *qps = sw + 4 * B, *st = qps + B;
  abi_ok(qloco_servo_force_block_body(&prm_, batch_, d_ws_, coma, com, rf, lf, bp, ft, rs, md, y,
                                      cnt, J, rm, ve, Fs, Fl, g, tau, sw, qps, st,
                                      body_.get(), arena_.stream()),
         "qloco_servo_force_block_body");
  arena_.download(F_sum.data(), Fs, sizeof(double) * 6 * B);
  arena_.download(Force_L_R.data(), Fl, sizeof(double) * 6 * B);
  arena_.download(grf_opt.data(), g, sizeof(double) * 12 * B);
  arena_.download(Legs_torque.data(), tau, sizeof(double) * 12 * B);
  arena_.download(swing.data(), sw, sizeof(int32_t) * 4 * B);
  arena_.download(qp_solution.data(), qps, sizeof(int32_t) * B);
  arena_.download(status.data(), st, sizeof(int32_t) * B);
  arena_.sync();
}

// ------------------------------------------------------------------------
// Go1ServoBatch
namespace {
// d_in_: q_mea 12 | quat 4 | gait 100 | y_offset 1; d_out_: q_cmd 12 | ctrl 25 | tau 12 | grf 12 | data 100
constexpr size_t kGI_Q = 0, kGI_QUAT = 12, kGI_GAIT = 16, kGI_Y = 116, kGI_N = 117;
constexpr size_t kGO_Q = 0, kGO_CTRL = 12, kGO_TAU = 37, kGO_GRF = 49, kGO_DATA = 61, kGO_N = 161;
}  // namespace

Go1ServoBatch::Go1ServoBatch(int batch, const qloco_go1_servo_params *p)
    : batch_(positive_batch(batch, "Go1ServoBatch")) {
  if (p) params = *p;
  else qloco_go1_servo_params_default(&params);
  const size_t B = batch;
  const int64_t ws = qloco_go1_servo_workspace_bytes(batch);
  if (ws < 0) throw Error("qloco_go1_servo_workspace_bytes", QLOCO_ERR_ARG);
  d_ws_ = arena_.alloc((size_t)ws);
  d_in_ = dalloc<double>(arena_, B * kGI_N);
  d_out_ = dalloc<double>(arena_, B * kGO_N);
  d_rec_ = dalloc<double>(arena_, B * QLOCO_GO1_SERVO_STATE);
  d_mode_ = dalloc<int32_t>(arena_, B);
  q_cmd.assign(B * 12, 0.0);
  state_to_MPC.assign(B * QLOCO_CTRL_MSG_LEN, 0.0);
  state_feedback.assign(B * QLOCO_CTRL_MSG_LEN, 0.0);
  Legs_torque.assign(B * 12, 0.0);
  grf_opt.assign(B * 12, 0.0);
  FR_angle_des.assign(B * 3, 0.0);
  FL_angle_des.assign(B * 3, 0.0);
  RR_angle_des.assign(B * 3, 0.0);
  RL_angle_des.assign(B * 3, 0.0);
  joint2simulation.assign(B * QLOCO_GO1_GAIT_DATA_LEN, 0.0);
  abi_ok(qloco_go1_servo_init(&params, batch_, d_ws_, arena_.stream()), "qloco_go1_servo_init");
  arena_.sync();
}

void Go1ServoBatch::tick(const double *q_mea, const double *quat, const double *gait,
                         const int32_t *gait_mode, const double *y_offset) {
  if (!q_mea || !quat || !gait || !gait_mode || !y_offset)
    throw Error("Go1ServoBatch::tick: null argument", QLOCO_ERR_ARG);
  const size_t B = batch_;
  arena_.upload(d_in_ + kGI_Q * B, q_mea, sizeof(double) * 12 * B);
  arena_.upload(d_in_ + kGI_QUAT * B, quat, sizeof(double) * 4 * B);
  arena_.upload(d_in_ + kGI_GAIT * B, gait, sizeof(double) * QLOCO_GAIT_MSG_LEN * B);
  arena_.upload(d_in_ + kGI_Y * B, y_offset, sizeof(double) * B);
  arena_.upload(d_mode_, gait_mode, sizeof(int32_t) * B);
  abi_ok(qloco_go1_servo_tick_body(&params, batch_, d_ws_, n_count, d_in_ + kGI_Q * B,
                                   d_in_ + kGI_QUAT * B, d_in_ + kGI_GAIT * B, d_mode_,
                                   d_in_ + kGI_Y * B, d_out_ + kGO_Q * B, d_out_ + kGO_CTRL * B,
                                   d_out_ + kGO_TAU * B, d_out_ + kGO_GRF * B, nullptr,
                                   d_out_ + kGO_DATA * B, body_.get(), arena_.stream()),
         "qloco_go1_servo_tick_body");
  arena_.download(q_cmd.data(), d_out_ + kGO_Q * B, sizeof(double) * 12 * B);
  arena_.download(state_to_MPC.data(), d_out_ + kGO_CTRL * B, sizeof(double) * QLOCO_CTRL_MSG_LEN * B);
  arena_.download(Legs_torque.data(), d_out_ + kGO_TAU * B, sizeof(double) * 12 * B);
  arena_.download(grf_opt.data(), d_out_ + kGO_GRF * B, sizeof(double) * 12 * B);
  arena_.download(joint2simulation.data(), d_out_ + kGO_DATA * B,
                  sizeof(double) * QLOCO_GO1_GAIT_DATA_LEN * B);
  std::vector<double> rec(B * QLOCO_GO1_SERVO_STATE);
  get_state(rec.data());  // syncs
  for (size_t b = 0; b < B; ++b) {
    const double *r = rec.data() + b * QLOCO_GO1_SERVO_STATE;
    for (int k = 0; k < 3; ++k) {
      FR_angle_des[3 * b + k] = r[75 + k];
      FL_angle_des[3 * b + k] = r[78 + k];
      RR_angle_des[3 * b + k] = r[81 + k];
      RL_angle_des[3 * b + k] = r[84 + k];
    }
    state_feedback[QLOCO_CTRL_MSG_LEN * b] = r[230];
  }
  ++n_count;
}

void Go1ServoBatch::get_state(double *state) {
  if (!state) throw Error("Go1ServoBatch::get_state: null argument", QLOCO_ERR_ARG);
  abi_ok(qloco_go1_servo_get_state(batch_, d_ws_, d_rec_, arena_.stream()), "qloco_go1_servo_get_state");
  arena_.download(state, d_rec_, sizeof(double) * (size_t)batch_ * QLOCO_GO1_SERVO_STATE);
  arena_.sync();
}

void Go1ServoBatch::set_state(const double *state) {
  if (!state) throw Error("Go1ServoBatch::set_state: null argument", QLOCO_ERR_ARG);
  arena_.upload(d_rec_, state, sizeof(double) * (size_t)batch_ * QLOCO_GO1_SERVO_STATE);
  abi_ok(qloco_go1_servo_set_state(batch_, d_ws_, d_rec_, arena_.stream()), "qloco_go1_servo_set_state");
  arena_.sync();
}

}  // namespace qloco

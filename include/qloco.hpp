/*
 * qloco.hpp -- C++ host shim with the reference's class / method signatures.
 *
 * Drop-in layer for the ROS control loops of jtdingx/quadrupedal_loco: the
 * classes keep the reference's names, argument meaning and result members,
 * and run the solves on the MI355X through the C ABI of qloco.h
 * (libqloco_host.so -> libqloco.so).  Eigen fixed-size matrices of the
 * reference become column-major `double` arrays of the same shape (Eigen's
 * default storage: pass `m.data()`); INTEGRATION.md shows the three-line
 * adapters for the Eigen call sites.
 *
 *   QPsolverGpu / QPBaseClassGpu  <- QPsolver / QPsolver_EiQuadProg /
 *                                    QPBaseClass (rt_mpc_qp/src/QP/QPBaseClass.h:19-73,
 *                                    QPBaseClass.cpp:20-152)
 *   Dynamiccclass                 <- go1_rt_control Dynamiccclass
 *                                    (dynmics_compute.h:59-76; servo.cpp:1224-1228)
 *   PRMPCClass                    <- rt_mpc_qp PRMPCClass::body_theta_mpc / Indexfind
 *                                    (PRMPCClass.h:69-71; gait_fast.cpp:620)
 *   ConvexMpcBatch                <- A1RobotControl::compute_grf MPC branch +
 *                                    ConvexMpc (A1RobotControl.cpp:452-600)
 *   A1RobotControlBatch           <- A1RobotControl::update_plan / generate_swing_legs_ctrl /
 *                                    compute_joint_torques (a1_cpp_open_source/src/
 *                                    A1RobotControl.cpp:149-324) and the terrain-pitch
 *                                    preamble of compute_grf (:341-380)
 *   A1BasicEKFBatch               <- A1BasicEKF (a1_cpp_open_source/src/A1BasicEKF.h:25-72;
 *                                    GazeboA1ROS.cpp:204-209)
 *   Go1ServoBatch                 <- one iteration of the go1 sim servo loop (go1_rt_control/
 *                                    src/servo_control/servo.cpp:675-1330)
 *   NLPClassBatch                 <- NLPClass::step_timing_opti_loop + Foot_trajectory_solve_mod2
 *   NLPRTControlBatch             <- NLPRTControlClass::WalkingReactStepping and the node loop of
 *                                    gait_nlp_kmp.cpp:101-158 (the /MPC/Gait row)
 *   NLPStepTimingBatch            <- NLPClass::step_timing_opti_loop (mosek_nlp_kmp/src/NLP/
 *                                    NLPClass_sqp.cpp:693-1102; NLPRTControlClass.cpp:445)
 *   Kinematicclass                <- go1_rt_control Kinematicclass
 *                                    (Kinematics.h:30-61; servo.cpp:734-741, :1038-1051)
 *   ServoForceBlock               <- the go1 servo loop's force block (servo.cpp:1052-1243)
 *   RtMpcNode                     <- the rt_mpc_qp node loop (gait_fast.cpp:79-735):
 *                                    subscriber callbacks + one 100 Hz iteration
 *
 * Every class is batched over B independent robots (B = 1 is the drop-in
 * case).  Host arrays are staged to the device on the object's HIP stream;
 * device-pointer entry points skip the staging.  Failures of the device
 * path throw qloco::Error (there is no CPU fallback); solver outcomes are
 * reported like the reference (NaN-free X / qp_solution flags).
 */
#pragma once

#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "qloco.h"

namespace qloco {

class Error : public std::runtime_error {
 public:
  Error(const std::string &what, int status);
  int status;
};

// Owned device memory + one HIP stream (created on construction).
class DeviceArena {
 public:
  DeviceArena();
  ~DeviceArena();
  DeviceArena(const DeviceArena &) = delete;
  DeviceArena &operator=(const DeviceArena &) = delete;
  void *alloc(size_t bytes);        // persistent block, freed with the arena
  void release(void *p);            // free one block early (no-op on nullptr)
  void upload(void *dev, const void *host, size_t bytes);
  void download(void *host, const void *dev, size_t bytes);
  void sync();
  void *stream() const { return stream_; }

 private:
  void *stream_ = nullptr;
  std::vector<void *> blocks_;
};

// Per-robot rows (set_bodies / set_models) in a block of the owner's arena.
// set() copies `batch` host rows to the device now, allocating the block on
// first use; nullptr switches the rows off and keeps the block.  get() is the
// pointer the C ABI takes: nullptr while the rows are off.
template <class T>
class DeviceRows {
 public:
  void set(DeviceArena &arena, int batch, const T *host_rows) {
    on_ = host_rows != nullptr;
    if (!on_) return;
    const size_t bytes = sizeof(T) * (size_t)batch;
    if (!dev_) dev_ = static_cast<T *>(arena.alloc(bytes));
    arena.upload(dev_, host_rows, bytes);
    arena.sync();  // the caller's rows may go away after the call
  }
  const T *get() const { return on_ ? dev_ : nullptr; }

 private:
  T *dev_ = nullptr;
  bool on_ = false;
};

// ------------------------------------------------------------------------
// QPsolver / QPsolver_EiQuadProg (QPBaseClass.cpp:20-56): min 0.5 x'Gx + g0'x
// s.t. CE'x + ce0 = 0, CI'x + ci0 >= 0 (EiQuadProg.hpp:15-36), quirk-compatible
// Goldfarb-Idnani in fp64 on the GPU.  Capacity n <= 64, p <= 64, m <= 320
// (qloco_gi_limits; the reference's QPBaseClass asserts nVars <= 60, nIneq <=
// 300, QPBaseClass.cpp:111-112): gi_kernel up to n, p <= 16 / m <= 64,
// gi_wide_kernel above that.
class QPsolverGpu {
 public:
  explicit QPsolverGpu(int max_batch = 1);
  ~QPsolverGpu();
  void resize(const int &nVar, const int &nEq, const int &nIneq);
  // One QP; matrices column-major (G n*n, CE n*p, CI n*m).  Returns the cost
  // (+inf when infeasible, as solve_quadprog).  G is left unchanged.
  double solve(const double *G, const double *g0, const double *CE, const double *ce0,
               const double *CI, const double *ci0, double *X);
  // B QPs of the current size; host arrays of B consecutive instances.
  void solve_batch(int batch, const double *G, const double *g0, const double *CE,
                   const double *ce0, const double *CI, const double *ci0, double *X,
                   double *f, int32_t *status);
  int last_status() const { return last_status_; }
  int last_iterations() const { return last_iters_; }

 private:
  int n_ = 0, p_ = 0, m_ = 0, cap_ = 0, max_batch_;
  int an_ = 0, ap_ = 0, am_ = 0;  // sizes the current device blocks were allocated for
  DeviceArena arena_;
  double *dG_ = nullptr, *dg0_ = nullptr, *dCE_ = nullptr, *dce0_ = nullptr, *dCI_ = nullptr,
         *dci0_ = nullptr, *dX_ = nullptr, *df_ = nullptr;
  int32_t *dst_ = nullptr, *dit_ = nullptr;
  int last_status_ = 0, last_iters_ = 0;
  void ensure(int batch);
};

// QPBaseClass (QPBaseClass.h:19-73): owns the QP buffers, solveQP() reports
// success as "no NaN in X" and ignores the cost (QPBaseClass.cpp:126-152).
class QPBaseClassGpu {
 public:
  std::vector<double> G, g0, CE, ce0, CI, ci0, X;
  int nVars = 0, nEq = 0, nIneq = 0;
  void resizeQP(const int &nVars, const int &nEq, const int &nIneq);
  bool solveQP();

 private:
  QPsolverGpu solver_{1};
};

// ------------------------------------------------------------------------
// Dynamiccclass (go1_rt_control/src/whole_body_dynamics/dynmics_compute.h:59-76).
// force_distribution + force_opt of robot r are staged; the batch runs on
// the GPU when force_opt is called for the last robot (robot == batch-1),
// or explicitly with run().  For batch == 1 this is exactly the reference's
// call sequence (servo.cpp:1224-1228).  Leg order FR, FL, RR, RL.
class Dynamiccclass {
 public:
  explicit Dynamiccclass(int batch = 1, const qloco_force_params *params = nullptr);
  void force_distribution(const double com_des[3], const double leg_des[12],
                          const double F_force_des[6], int mode, double y_coefficient,
                          const double rfoot_des[3], const double lfoot_des[3], int robot = 0);
  void force_opt(const double base_p[3], const double FR_p[3], const double FL_p[3],
                 const double RR_p[3], const double RL_p[3], const double FT_total_des[6],
                 int mode, int right_support, double y_coefficient, int robot = 0);
  void run();
  // Per-robot bodies (qloco_force_body, include/qloco.h section 3): host_rows
  // holds B rows, copied to the device now (the device rows are allocated on
  // first use); run() then solves robot b with
  // its row's alpha, beta, gamma, fz_max and mu.  nullptr returns to params.  A robot
  // with a refused row gets status QLOCO_ERR_ARG and keeps its members.
  void set_bodies(const qloco_force_body *host_rows) { body_.set(arena_, batch_, host_rows); }
  // compute_joint_torques for all legs of all robots (dynmics_compute.cpp:109-138)
  void compute_joint_torques(const double *Jaco /*B*4*9*/, const int32_t *swing /*B*4*/,
                             const double *p_des, const double *p_est, const double *pv_des,
                             const double *pv_est, double *tau /*B*12*/);
  // reference result members, B consecutive records
  std::vector<double> grf_opt;      // 12 per robot
  std::vector<double> F_leg_ref;    // 3x4 col-major per robot
  std::vector<double> F_leg_guess;  // 12 per robot
  std::vector<int32_t> qp_solution, status, iters;
  int batch() const { return batch_; }

 private:
  int batch_;
  qloco_force_params prm_;
  DeviceArena arena_;
  std::vector<double> h_com_, h_leg_, h_F_, h_rf_, h_lf_, h_base_, h_feet_, h_FT_, h_y_;
  std::vector<int32_t> h_mode_, h_rs_;
  double *d_com_, *d_leg_, *d_F_, *d_rf_, *d_lf_, *d_base_, *d_feet_, *d_FT_, *d_y_, *d_Fref_,
      *d_grf_, *d_guess_;
  int32_t *d_mode_, *d_rs_, *d_qps_, *d_st_, *d_it_;
  int32_t *d_ord_;           // grouped-launch workspace (qloco_force_order_ws_len)
  DeviceRows<qloco_force_body> body_;  // set_bodies' rows
  double *d_jt_ = nullptr;   // joint-torque staging (allocated on first use)
  int32_t *d_sw_ = nullptr;
};

// ------------------------------------------------------------------------
// PRMPCClass::body_theta_mpc (rt_mpc_qp/src/FastMPC/PRMPCClass.h:69-71): the
// 8-variable body-inclination QP with the reference's member state
// (thetaxk/thetayk, V_ini, bjx1/bjx2/t_yu), one record per robot.
class PRMPCClass {
 public:
  explicit PRMPCClass(int batch = 1);
  // Eigen 2x5 / 3x5 inputs as column-major arrays; returns the 14-vector
  // [thx0, thy0, taux0, tauy0, zmpx0, zmpy0, thx1, thy1, zmpx1, zmpy1, thx2, thy2,
  //  zmpx2, zmpy2] (PRMPCClass.cpp:696-709).  Nrtfoorpr_gen is unused by the
  // reference body and accepted for signature compatibility.
  std::array<double, 14> body_theta_mpc(int i, const double bodyangle_state[4],
                                        const double zmp_ref[10], const double angle_ref[10],
                                        const double rfoot_ref[10], const double lfoot_ref[10],
                                        const double comacc_ref[15],
                                        const double Nrtfoorpr_gen[9] = nullptr);
  // B robots at once (host arrays, B consecutive records each); com_traj B*14.
  void body_theta_mpc_batch(const int32_t *i, const double *bodyangle_state, const double *zmp_ref,
                            const double *angle_ref, const double *rfoot_ref,
                            const double *lfoot_ref, const double *comacc_ref, double *com_traj);
  int Indexfind(double goal_P);
  std::vector<double> state;  // QLOCO_BODY_STATE_LEN doubles per robot (host mirror)

 private:
  int batch_;
  DeviceArena arena_;
  double *d_state_, *d_in_, *d_traj_, *d_t_;
  int32_t *d_i_, *d_st_, *d_j_;
};

// ------------------------------------------------------------------------
// A1RobotControl::compute_grf, MPC branch (A1RobotControl.cpp:452-600) over B
// robots: x0 and the desired trajectory are built exactly as :459-497, the
// batched fused build + OSQP-algorithm ADMM runs on the GPU, and the forces
// come back in the body frame (root_rot_mat' u, :596-599).  A leg whose
// solution is NaN keeps its previous output (the reference's isnan guard).
// Like the reference's member OsqpEigen::Solver (A1RobotControl.h:67, set up
// once with warm start on, then update* + solve every tick, :556-578), each
// robot's solver persists across compute_grf calls (spec.warm_start = 2, the
// per-robot record on the device) and, by default, solves the reference's
// literal 12N-variable QP (spec.literal_full_qp = 1), so every call after
// the first takes OSQP's update path as the reference's does, contact
// changes included; reset() forgets it.  Pass a spec with warm_start = 0
// for independent cold solves, literal_full_qp = 0 for the faster
// stance-only reduction (same optimum; DESIGN.md §3c for its persistence).
struct A1MpcState {                // the A1CtrlStates fields compute_grf reads
  double root_euler[3], root_pos[3], root_ang_vel[3], root_lin_vel[3];
  double root_rot_mat[9];          // col-major; used for root_lin_vel_d_world
  double root_euler_d[3], root_pos_d[3], root_ang_vel_d[3], root_lin_vel_d[3];
  double foot_pos_abs[12];         // 3x4 col-major, legs FL, FR, RL, RR
  bool contacts[4];
};

class ConvexMpcBatch {
 public:
  ConvexMpcBatch(int batch, const qloco_srbd_spec *spec = nullptr);
  // Multi-GPU (include/qloco.h §10): this object is rank `rank` of `world`
  // (one process or thread per GPU, its device current) over a global batch
  // of `total` robots.  It owns the shard qloco_mgpu_shard assigns
  // (shard_first + k * shard_stride, k < shard_count): compute_grf takes and
  // returns that shard, and one RCCL all-gather per call leaves every
  // robot's forces (same frame, same NaN guard) in all_forces(), total * 12,
  // on every rank.  comm_id: qloco_mgpu_unique_id() on rank 0, shipped to
  // the other ranks by the caller (QLOCO_MGPU_ID_BYTES bytes).
  ConvexMpcBatch(int64_t total, int world, int rank, const uint8_t *comm_id,
                 int shard_mode = QLOCO_SHARD_CONTIGUOUS, const qloco_srbd_spec *spec = nullptr);
  ~ConvexMpcBatch();
  ConvexMpcBatch(const ConvexMpcBatch &) = delete;
  ConvexMpcBatch &operator=(const ConvexMpcBatch &) = delete;
  const std::vector<double> &all_forces() const { return all_forces_; }
  int64_t shard_first = 0, shard_count = 0, shard_stride = 1;
  // foot_forces_grf: B * 12 (3x4 col-major per robot), in/out
  void compute_grf(const A1MpcState *states, double *foot_forces_grf);
  // device-resident form (inputs already in HBM): thin wrapper of qloco_srbd_solve_ex
  void solve_device(const float *x0, const float *x_ref, const float *feet,
                    const uint8_t *contacts, float *u0, int32_t *status, int32_t *iters);
  void reset();  // fresh solvers (the next call sets each one up again)
  // Per-robot bodies (qloco_srbd_model, include/qloco.h): host_rows holds one
  // row per robot of this object -- B rows, or this rank's shard_count rows in
  // the multi-GPU form, in compute_grf's order -- copied to the device now;
  // compute_grf and solve_device then solve robot b with its row's mass,
  // inertia, mu and fz_min / fz_max in place of the spec's.  nullptr returns
  // to the spec's body.  A robot with an invalid row gets status
  // QLOCO_ERR_ARG and keeps its previous forces (the NaN guard).
  void set_models(const qloco_srbd_model *host_rows) { model_.set(arena_, batch_, host_rows); }
  // settings / weights may be edited between calls; horizon and warm_start
  // size the device buffers and are fixed at construction (a changed value
  // throws qloco::Error on the next call)
  qloco_srbd_spec spec;
  std::vector<int32_t> status, iters;

 private:
  void check_spec() const;
  int batch_;
  int horizon_ = 0, warm_mode_ = 0;
  DeviceArena arena_;
  float *d_x0_, *d_xr_, *d_feet_, *d_u0_, *d_rec_ = nullptr;
  DeviceRows<qloco_srbd_model> model_;  // set_models' rows
  uint8_t *d_ct_;
  int32_t *d_st_, *d_it_;
  // multi-GPU form
  qloco_mgpu *mg_ = nullptr;
  int64_t total_ = 0;
  float *d_u0_all_ = nullptr;
  int32_t *d_st_all_ = nullptr, *d_it_all_ = nullptr;
  std::vector<double> all_forces_;
};

// ------------------------------------------------------------------------
// A1RobotControl::compute_grf, QP branch (stance_leg_control_type == 0,
// A1RobotControl.cpp:383-450) over B robots: the A1CtrlStates fields it
// reads, the weights / gains of qloco_a1_params, one cold OSQP solve per
// robot (fp64, qloco_a1_qp_solve), forces in the body frame.
struct A1QpState {
  double root_pos[3], root_pos_d[3], root_euler[3], root_euler_d[3];
  double root_lin_vel[3], root_lin_vel_d[3], root_ang_vel[3], root_ang_vel_d[3];
  double root_rot_mat[9], root_rot_mat_z[9];  // col-major
  double foot_pos_abs[12];                    // 3x4 col-major, legs FL, FR, RL, RR
  bool contacts[4];
};

class A1QpBatch {
 public:
  // throws Error(QLOCO_ERR_ARG) for parameters qloco_a1_params_check refuses
  A1QpBatch(int batch, const qloco_a1_params *params = nullptr);
  // foot_forces_grf: B * 12 (3x4 col-major per robot)
  void compute_grf(const A1QpState *states, double *foot_forces_grf);
  // Per-robot bodies (qloco_a1_body, include/qloco.h section 9): host_rows
  // holds B rows, in compute_grf's order, copied to the device now;
  // compute_grf then solves robot b with its row's gains, mass, weights, mu
  // and f_min / f_max in place of params' (the solver settings stay params').
  // nullptr returns to params.  A robot with an invalid row gets status
  // QLOCO_ERR_ARG and NaN forces.
  void set_bodies(const qloco_a1_body *host_rows) { body_.set(arena_, batch_, host_rows); }
  qloco_a1_params params;
  std::vector<int32_t> status, iters;

 private:
  int batch_;
  DeviceArena arena_;
  double *d_state_, *d_forces_;
  DeviceRows<qloco_a1_body> body_;  // set_bodies' rows
  uint8_t *d_ct_;
  int32_t *d_st_, *d_it_;
};

// ------------------------------------------------------------------------
// A1BasicEKF (A1BasicEKF.h:25-72) over B robots, as GazeboA1ROS::main_update
// drives it (GazeboA1ROS.cpp:204-209): init_state on the first tick,
// update_estimation afterwards.  A1EstState carries the A1CtrlStates fields
// the filter reads (movement_mode .. foot_force) and writes (estimated_* and
// root_pos / root_lin_vel); x and P stay on the device (qloco_a1_ekf_*).
struct A1EstState {
  int movement_mode;
  double root_rot_mat[9];                   // 3x3 col-major
  double imu_acc[3], imu_ang_vel[3];
  double foot_pos_rel[12], foot_vel_rel[12];  // 3x4 col-major, legs FL, FR, RL, RR
  double foot_force[4];
  bool estimated_contacts[4];
  double estimated_root_pos[3], estimated_root_vel[3];
  double root_pos[3], root_lin_vel[3];
};

class A1BasicEKFBatch {
 public:
  A1BasicEKFBatch(int batch, const qloco_a1_ekf_params *params = nullptr);
  A1BasicEKFBatch(int batch, bool assume_flat_ground);
  bool is_inited() const { return filter_initialized_; }
  void init_state(const A1EstState *states);
  void update_estimation(A1EstState *states, double dt);
  // dense x (B * 18) and P (B * 324, col-major) of every filter
  void get_state(double *x, double *P);
  qloco_a1_ekf_params params;
  int batch() const { return batch_; }

 private:
  int batch_;
  bool filter_initialized_ = false;
  DeviceArena arena_;
  void *d_ws_;
  double *d_in_, *d_out_;
  int32_t *d_mode_;
  uint8_t *d_ct_;
  void stage(const A1EstState *states, double dt);
};

// ------------------------------------------------------------------------
// A1RobotControl's update_plan, generate_swing_legs_ctrl, terrain-pitch
// preamble of compute_grf and compute_joint_torques (A1RobotControl.cpp:149-380)
// over B robots.  A1CtrlState carries the A1CtrlStates fields those functions
// read and write, under their names; the members that persist from tick to
// tick (gait counters, *_last_time, the moving-window filters, ...) stay on the
// device (qloco_a1_ctrl_*) and are mirrored into the host fields after every
// call.  The reference calls update_plan and generate_swing_legs_ctrl back to
// back (GazeboA1ROS.cpp:199-202): update_plan only stages its inputs, the
// device call runs in generate_swing_legs_ctrl, which then fills the outputs
// of both (plan_contacts, gait_counter and the foot_pos_target_* arrays
// included).  Calling generate_swing_legs_ctrl without update_plan throws.
struct A1CtrlState {
  int movement_mode;
  double root_pos[3], root_lin_vel[3], root_lin_vel_d[3], root_euler_d[3];
  double root_rot_mat[9], root_rot_mat_z[9];  // 3x3 col-major
  double foot_pos_abs[12];                    // 3x4 col-major, legs FL, FR, RL, RR
  double foot_force[4];
  double j_foot[36];            // the four 3x3 diagonal blocks, each col-major
  double foot_forces_grf[12];
  // written
  double gait_counter[4];
  bool plan_contacts[4], early_contacts[4], contacts[4];
  double foot_pos_target_rel[12], foot_pos_target_abs[12], foot_pos_target_world[12];
  double foot_pos_cur[12], foot_forces_kin[12], foot_pos_recent_contact[12];
  double terrain_pitch_angle;
  double joint_torques[12];
};

class A1RobotControlBatch {
 public:
  A1RobotControlBatch(int batch, const qloco_a1_ctrl_params *params = nullptr);
  void update_plan(A1CtrlState *states, double dt);               // stages only
  void generate_swing_legs_ctrl(A1CtrlState *states, double dt);  // plan + swing on the device
  void compute_terrain_pitch(A1CtrlState *states);  // writes root_euler_d[1], terrain_pitch_angle
  void compute_joint_torques(A1CtrlState *states);
  // dense member state, B * QLOCO_A1_CTRL_STATE doubles (include/qloco.h section 13)
  void get_state(double *state);
  void reset();
  qloco_a1_ctrl_params params;
  int batch() const { return batch_; }

 private:
  int batch_;
  bool staged_ = false;
  double staged_dt_ = 0.0;
  DeviceArena arena_;
  void *d_ws_;
  double *d_in_, *d_out_, *d_rec_;
  int32_t *d_mode_;
  uint8_t *d_ct_;
};

// ------------------------------------------------------------------------
// NLPClass::step_timing_opti_loop (mosek_nlp_kmp/src/NLP/NLPClass.h:66-67,
// NLPClass_sqp.cpp:693-1102; called at NLPRTControlClass.cpp:445) for B robots
// -> qloco_nlp_step_timing.  The constructor runs FootStepInputs + Initialize.
// estimated_state is the reference's 18-vector (elements 0..5 are read), the
// foot-location feedbacks its 3-vectors (x, y are read); `lamda` and
// `stopwalking` are accepted and unused, as in the reference (they only reach
// CoM_height_solve).  The 38-vector com_traj comes back per robot (row per
// robot, the reference's slot order).  Slots this library does not compute --
// _comz / _comvz / _comaz and everything derived from them, ZMP and DCM:
// 2, 5, 8, 9..20, 23, 26 -- are quiet NaN on every call, never stale.  Slots
// 28..33 are NaN too on the plan's last step, where the reference reads
// _footx_ref past its end.
class NLPStepTimingBatch {
 public:
  static constexpr int kComTraj = 38;
  NLPStepTimingBatch(int batch, double stepwidth, double steplength, double stepheight,
                     const qloco_nlp_params *params = nullptr);
  // B = 1: the reference's signature, returns com_traj
  std::array<double, 38> step_timing_opti_loop(int i, const double estimated_state[18],
                                               const double Rfoot_location_feedback[3],
                                               const double Lfoot_location_feedback[3], double lamda,
                                               bool stopwalking);
  // B robots: estimated_state[B*18], feedbacks[B*3] -> com_traj[B*38]
  void step_timing_opti_loop(int i, const double *estimated_state, const double *Rfoot_location_feedback,
                             const double *Lfoot_location_feedback, double lamda, bool stopwalking,
                             double *com_traj);
  // dense member state, B * QLOCO_NLP_STATE doubles (include/qloco.h section 14)
  void get_state(double *state);
  void set_state(const double *state);
  // of the last call, per robot: QLOCO_OK, QLOCO_NAN, QLOCO_NLP_FINISHED, QLOCO_BAD_SIZE
  const std::vector<int32_t> &status() const { return status_; }
  // device views for qloco_support_phase: _ts / _tx, B x 27 doubles each
  const double *ts_device() const { return (const double *)d_ws_; }
  const double *tx_device() const { return (const double *)d_ws_ + (size_t)batch_ * QLOCO_NLP_STEPS; }
  qloco_nlp_params params;
  int batch() const { return batch_; }

 private:
  int batch_;
  double stepheight_;
  DeviceArena arena_;
  void *d_ws_;
  double *d_in_, *d_out_, *d_rec_;
  int32_t *d_i_, *d_int_;
  std::vector<int32_t> status_;
};

// ------------------------------------------------------------------------
// NLPClass up to the class boundary for B robots -> qloco_nlp_tick (section
// 15): step_timing_opti_loop returns the fully populated 38-vector (slots
// 28..33 are NaN only on the plan's last step, where the reference reads
// _footx_ref past its end), Foot_trajectory_solve_mod2 the 18-vector of the
// same tick, and right_support is the member the reference leaves behind.
// The device call runs in step_timing_opti_loop with the `stopwalking` it is
// given; Foot_trajectory_solve_mod2 returns what that call computed and throws
// when j_index or stopwalking differ from it, or when no tick preceded it
// (NLPRTControlClass.cpp:445-459 calls the two back to back with the same
// arguments).  `lamda` is accepted and unused, as in the reference.
// Zmp_distributor and the _state_generate_interpo packing are NLPRTControlBatch's.
class NLPClassBatch {
 public:
  static constexpr int kComTraj = 38, kFootTraj = 18;
  NLPClassBatch(int batch, double stepwidth, double steplength, double stepheight,
                const qloco_nlp_params *params = nullptr, const qloco_nlp_tick_params *tick_params = nullptr);
  // B = 1: the reference's signatures
  std::array<double, 38> step_timing_opti_loop(int i, const double estimated_state[18],
                                               const double Rfoot_location_feedback[3],
                                               const double Lfoot_location_feedback[3], double lamda,
                                               bool stopwalking);
  std::array<double, 18> Foot_trajectory_solve_mod2(int j_index, bool stopwalking);
  // B robots: estimated_state[B*18], feedbacks[B*3] -> com_traj[B*38]; rlfoot_traj[B*18]
  void step_timing_opti_loop(int i, const double *estimated_state, const double *Rfoot_location_feedback,
                             const double *Lfoot_location_feedback, double lamda, bool stopwalking,
                             double *com_traj);
  void Foot_trajectory_solve_mod2(int j_index, bool stopwalking, double *rlfoot_traj);
  int right_support = 0;                        // robot 0, after the last tick (:493)
  std::vector<int32_t> right_support_batch;     // every robot
  // dense member state: B * QLOCO_NLP_STATE and B * QLOCO_NLP_TICK_STATE doubles
  void get_state(double *nlp_state, double *tick_state);
  void set_state(const double *nlp_state, const double *tick_state);
  const std::vector<int32_t> &status() const { return status_; }
  qloco_nlp_params params;
  qloco_nlp_tick_params tick_params;
  int batch() const { return batch_; }

 private:
  int batch_, last_i_ = 0;
  bool last_stop_ = false, have_tick_ = false;
  DeviceArena arena_;
  void *d_ws_, *d_tws_;
  double *d_in_, *d_out_, *d_rec_, *d_trec_;
  int32_t *d_i_, *d_int_;
  std::vector<int32_t> status_;
  std::vector<double> foot_;
};

// ------------------------------------------------------------------------
// NLPRTControlClass (mosek_nlp_kmp/src/NLPRTControl/NLPRTControlClass.cpp) with
// the node loop around it (gait_nlp_kmp.cpp:101-158), B robots: the start latch
// and loop counter, the branch of WalkingReactStepping (not started, squat,
// walking, over time), the planner tick, Zmp_distributor and the 100-slot
// /MPC/Gait row, in one call with no host step (qloco_nlp_node_tick).  The
// constructor mirrors NLPRTControlClass(): the "go1" step inputs (:63-80) and
// the member setup (:86-185).  StartWalking / StopWalking are not modelled: the
// node never calls them.
class NLPRTControlBatch {
 public:
  static constexpr int kRow = QLOCO_GAIT_MSG_LEN;
  explicit NLPRTControlBatch(int batch = 1, double stepheight = 0.0, const qloco_nlp_params *params = nullptr,
                             const qloco_nlp_tick_params *tick_params = nullptr,
                             const qloco_nlp_node_params *node_params = nullptr);
  // B = 1, the reference's signature.  The node loop passes its counter and its
  // latch; the device keeps both per robot and advances them from msg[0] > 0, so
  // a call that continues the loop (walkdtime the last one or one more) costs no
  // extra transfer and any other rewrites the two members first.  estimated_state
  // is accepted and unused, as rt_nlp_gait passes its zero member instead (:445).
  // Once mpc_stop >= 1 the last row is returned, as the loop re-publishes it.
  std::array<double, 100> WalkingReactStepping(int walkdtime, bool start_mpc, const double estimated_state[18],
                                               const double Rfoot_location_feedback[3],
                                               const double Lfoot_location_feedback[3]);
  // B robots, device pointers, asynchronous on stream(): nrt_msg[B*25] (the
  // /rt2nrt/state rows: [0] > 0 starts a robot and advances its count) ->
  // gait_msg[B*100]; sched[B*8] and status[B] (int32) may be NULL.  Chains with
  // qloco_rt_tick and qloco_go1_servo_tick on the same buffers.
  void tick(const double *d_nrt_msg, double *d_gait_msg, int32_t *d_sched = nullptr, int32_t *d_status = nullptr);
  // dense member state: B * QLOCO_NLP_STATE, B * QLOCO_NLP_TICK_STATE and
  // B * QLOCO_NLP_NODE_STATE doubles
  void get_state(double *nlp_state, double *tick_state, double *node_state);
  void set_state(const double *nlp_state, const double *tick_state, const double *node_state);
  int right_support = 2;                         // robot 0, after the last B = 1 call
  double mpc_stop = 0;
  int status = QLOCO_OK;
  int32_t sched[QLOCO_NLP_NODE_SCHED_LEN] = {0};
  qloco_nlp_params params;
  qloco_nlp_tick_params tick_params;
  qloco_nlp_node_params node_params;
  int batch() const { return batch_; }
  void *stream() const { return arena_.stream(); }
  void sync() { arena_.sync(); }

 private:
  int batch_, count_ = 0;
  bool latch_ = false;
  DeviceArena arena_;
  void *d_ws_, *d_tws_, *d_nws_;
  double *d_msg_, *d_row_, *d_rec_, *d_trec_, *d_nrec_;
  int32_t *d_int_;
};

// ------------------------------------------------------------------------
// Kinematicclass (go1_rt_control/src/kinematics/Kinematics.h:30-61).  The
// per-leg methods keep the reference's signatures and leave the Jacobian of
// the last evaluation in Jacobian_kin (3x3 col-major), as the servo reads it
// (servo.cpp:735, :1039); the batch methods run n legs in one launch and are
// the intended use on the GPU (one leg per call is a host<->device round trip).
// feet_flag: 0 FR, 1 FL, 2 RR, 3 RL.  body_R = (roll, pitch, yaw).
class Kinematicclass {
 public:
  explicit Kinematicclass(int max_legs = 4);
  std::array<double, 3> Forward_kinematics(const double q_joint[3], int feet_flag);
  std::array<double, 3> Forward_kinematics_g(const double body_P[3], const double body_R[3],
                                             const double q_joint[3], int feet_flag);
  std::array<double, 3> Inverse_kinematics(const double pos_des[3], const double q_ini[3],
                                           int feet_flag);
  std::array<double, 3> Inverse_kinematics_g(const double body_P[3], const double body_R[3],
                                             const double pos_des[3], const double q_ini[3],
                                             int feet_flag);
  // n legs (host arrays, row layout of qloco_leg_fk / qloco_leg_ik); body_p /
  // body_r both NULL for the hip frame.  jac / pos_out / updates may be NULL.
  void forward_batch(int n, const double *q, const int32_t *leg, const double *body_p,
                     const double *body_r, double *pos, double *jac);
  void inverse_batch(int n, const double *pos_des, const double *q_ini, const int32_t *leg,
                     const double *body_p, const double *body_r, double *q_out, double *pos_out,
                     double *jac, int32_t *updates);
  std::array<double, 9> Jacobian_kin{};  // after the last per-leg call
  std::array<double, 3> pos_cal{};       // FK at the last IK result (the reference's pos_cal)
  int last_updates = 0;                  // Newton steps of the last per-leg IK

 private:
  int cap_;
  DeviceArena arena_;
  double *d_a_, *d_b_, *d_p_, *d_r_, *d_q_, *d_pos_, *d_jac_;
  int32_t *d_leg_, *d_upd_;
  void ensure(int n);
};

// ------------------------------------------------------------------------
// The rt_mpc_qp node (unitree_ros/rt_mpc_qp/src/gait_fast.cpp) for B robots:
// the two subscriber callbacks store the latest /MPC/Gait (100 doubles,
// :79-89) and /control2rtmpc/state (25 doubles, :92-110) message of a robot;
// loop_once() runs one iteration of the 100 Hz loop (:505-735) -- reference
// interpolation, PRMPCClass contact schedule / swing-foot / foot-rotation
// generators, body_theta_mpc -- for every robot on the GPU (qloco_rt_tick)
// and leaves the outgoing messages in `traj` (/rtMPC/traj, 100 per robot)
// and `nrt` (/rt2nrt/state, 25 per robot; valid when published(robot)).
class RtMpcNode {
 public:
  explicit RtMpcNode(int batch = 1);
  void nrt_gait_sub_operation(const double msg[QLOCO_GAIT_MSG_LEN], int robot = 0);
  void control_gait_sub_operation(const double msg[QLOCO_CTRL_MSG_LEN], int robot = 0);
  void loop_once();
  bool published(int robot = 0) const { return sched[robot * QLOCO_RT_SCHED_LEN + 6] != 0; }
  std::vector<double> traj;     // B * 100
  std::vector<double> nrt;      // B * 25
  std::vector<int32_t> sched;   // B * QLOCO_RT_SCHED_LEN (bjx1, bjxx, t_end, counters, ...)
  int batch() const { return batch_; }

 private:
  int batch_;
  DeviceArena arena_;
  std::vector<double> gait_, ctrl_;
  void *d_ws_;
  double *d_gait_, *d_ctrl_, *d_traj_, *d_nrt_;
  int32_t *d_sched_;
};

// ------------------------------------------------------------------------
// The go1 servo loop's force block (servo.cpp:1052-1243, :1318) for B robots:
// one call per servo tick replaces the F_sum / F_lr_predict / swing-flag
// glue, Dynam.force_distribution + force_opt and the four
// compute_joint_torques calls.  Host arrays of B consecutive records; legs
// FR, FL, RR, RL; Jaco = the four Jacobian_kin (3x3 col-major) per robot.
class ServoForceBlock {
 public:
  explicit ServoForceBlock(int batch = 1, const qloco_force_params *params = nullptr);
  void step(const double *coma_des, const double *com_des, const double *rfoot_des,
            const double *lfoot_des, const double *body_p_des, const double *foot_des,
            const int32_t *right_support, const int32_t *gait_mode, const double *y_offset,
            const int32_t *count_in_rt_loop, const double *Jaco, const double *foot_rel_mea,
            const double *v_est_rel);
  // Per-robot bodies (qloco_force_body, include/qloco.h section 3): host_rows
  // holds B rows, copied to the device now (the device rows are allocated on
  // first use); step() then builds F_sum with
  // robot b's mass and momentum and solves with its row.  nullptr returns to params.  A robot
  // with a refused row gets status QLOCO_ERR_ARG and NaN grf_opt / Legs_torque.
  void set_bodies(const qloco_force_body *host_rows) { body_.set(arena_, batch_, host_rows); }
  std::vector<double> F_sum, Force_L_R, grf_opt, Legs_torque;  // 6, 6, 12, 12 per robot
  std::vector<int32_t> swing, qp_solution, status;             // 4, 1, 1 per robot
  int batch() const { return batch_; }

 private:
  int batch_;
  qloco_force_params prm_;
  DeviceArena arena_;
  void *d_ws_;
  double *d_in_, *d_out_;
  int32_t *d_iin_, *d_iout_;
  DeviceRows<qloco_force_body> body_;  // set_bodies' rows
};

// ------------------------------------------------------------------------
// One iteration of the go1 sim servo loop (servo.cpp:675-1330) for B robots
// started together (batch 1: the drop-in case).  The callbacks fill the three
// inputs, tick() runs the loop body on the device (qloco.h section 16) and
// leaves the reference's members, by their names, in host arrays (robot b's
// values at b * n); the publishers stay with the caller.  n_count is the
// node's loop counter, incremented by tick().
class Go1ServoBatch {
 public:
  explicit Go1ServoBatch(int batch = 1, const qloco_go1_servo_params *params = nullptr);
  // q_mea[B*12] (lowState.motorState[j].q), quat[B*4] (w, x, y, z), slow_mpc_gait[B*100]
  // (the latest /MPC/Gait row), gait_mode[B], y_offset[B]
  void tick(const double *q_mea, const double *quat, const double *slow_mpc_gait,
            const int32_t *gait_mode, const double *y_offset);
  // Per-robot bodies (qloco_force_body, include/qloco.h section 3): host_rows
  // holds B rows, copied to the device now (the device rows are allocated on
  // first use); the gait branch of tick() then
  // builds F_sum with robot b's mass and momentum and solves with its row.  nullptr returns to params.  A robot
  // with a refused row gets status QLOCO_ERR_ARG and NaN grf_opt / Legs_torque.
  void set_bodies(const qloco_force_body *host_rows) { body_.set(arena_, batch_, host_rows); }
  std::vector<double> q_cmd;           // lowCmd.motorCmd[j].q, B*12
  std::vector<double> state_to_MPC;    // the /control2rtmpc/state row published at :762, B*25
  std::vector<double> state_feedback;  // the member after the tick ([0] = t_int), B*25
  std::vector<double> Legs_torque, grf_opt;                                    // B*12
  std::vector<double> FR_angle_des, FL_angle_des, RR_angle_des, RL_angle_des;  // 12-vectors: B*3
  std::vector<double> joint2simulation;                                        // go1_gait_data, B*100
  int n_count = 0;
  // dense member state: B * QLOCO_GO1_SERVO_STATE doubles
  void get_state(double *state);
  void set_state(const double *state);
  qloco_go1_servo_params params;
  int batch() const { return batch_; }

 private:
  int batch_;
  DeviceArena arena_;
  void *d_ws_;
  double *d_in_, *d_out_, *d_rec_;
  int32_t *d_mode_;
  DeviceRows<qloco_force_body> body_;  // set_bodies' rows
};

}  // namespace qloco

/*
 * qloco.h -- C ABI of the MI355X-native batched convex-MPC solver
 * (libqloco.so).  Plain pointers and sizes only; no torch / Eigen types.
 *
 * Every entry point below replaces one interface of the reference
 * (jtdingx/quadrupedal_loco, paths relative to its root) and is batched over
 * independent instances.  Device entry points take DEVICE pointers that are
 * already resident in HBM plus a hipStream_t (passed as void*; NULL = the
 * default stream); they only enqueue work and return immediately.  Host
 * entry points (suffix _host) take host pointers and block.
 *
 * Layout conventions
 *  - instance-major ("AoS per field"): field f of instance b lives at
 *    ptr[b * len(f) + k]; one instance's data is contiguous, so the one
 *    wavefront that owns the instance reads it with coalesced loads.
 *  - small matrices mirror Eigen's default column-major storage.
 *  - SRBD leg order is ConvexMpc's FL, FR, RL, RR (A1CtrlStates.h:44-46);
 *    force-QP leg order is the Go1 servo's FR, FL, RR, RL (servo.cpp:1054-1058).
 *
 * Errors: every function returns a qloco_status (0 = success).  Per-instance
 * solver outcomes go to the status[] arrays, mirroring QPBaseClass::solveQP
 * (QPBaseClass.cpp:126-152), which reports failure only through NaN in X.
 */
#ifndef QLOCO_H
#define QLOCO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QLOCO_ABI_VERSION 1

typedef enum qloco_status {
  QLOCO_OK = 0,
  QLOCO_MAX_ITER = 1,          /* ADMM hit max_iter (OSQP_MAX_ITER_REACHED)          */
  QLOCO_INFEASIBLE = 2,        /* EiQuadProg returned +inf (EiQuadProg.cpp:394-400)   */
  QLOCO_NAN = 3,               /* non-finite solution                                 */
  QLOCO_BAD_SIZE = 4,          /* sizes outside the compiled limits                   */
  QLOCO_NOT_PD = 5,            /* Cholesky failed (EiQuadProg.cpp:507-510)            */
  QLOCO_DEGENERATE = 6,        /* dependent equalities (EiQuadProg.cpp:270-275)       */
  QLOCO_UB_PATH = 7,           /* reference reads an uninitialised index (:105-110)   */
  QLOCO_SOLVED_INACCURATE = 8, /* OSQP_SOLVED_INACCURATE                              */
  QLOCO_ERR_ARG = 100,         /* invalid argument (call-level); in a per-instance    */
                               /* status array only from qloco_srbd_solve_model: that */
                               /* instance's model row is invalid                     */
  QLOCO_ERR_DEVICE = 101,      /* HIP runtime error (call-level)                      */
  QLOCO_ERR_NO_GPU = 102       /* no gfx950 device visible                            */
} qloco_status;

const char *qloco_status_string(int status);
int qloco_abi_version(void);
/* last HIP error string of the calling thread (empty if none) */
const char *qloco_last_error(void);

/* ====================================================================== */
/* 1. SRBD convex MPC (Go1, N-step horizon, 12 contact forces)             */
/*    replaces ConvexMpc (a1_cpp_open_source/src/ConvexMpc.h:22-94,        */
/*    ConvexMpc.cpp:8-264) + the OSQP solve in                             */
/*    A1RobotControl::compute_grf (A1RobotControl.cpp:452-600)             */
/* ====================================================================== */
typedef struct qloco_srbd_spec {
  int32_t horizon;           /* N = PLAN_HORIZON (A1Params.h:26)                   */
  int32_t feet_per_step;     /* 0: feet[12] per instance (compute_grf); 1: [12N]   */
  int32_t contacts_per_step; /* 0: contacts[4] (ConvexMpc.cpp:232-249); 1: [4N]    */
  int32_t output_frame;      /* 0: u0 = QP solution (world);                        */
                             /* 1: R^T u0 per leg (compute_grf return, :596-599)    */
  float dt;                  /* mpc_dt = 0.0025 (A1RobotControl.cpp:469)            */
  float mass;                /* robot_mass                                           */
  float inertia[9];          /* trunk inertia, col-major                             */
  float q_weights[13];       /* ConvexMpc ctor q_weights_ (Q = diag(2q))             */
  float r_weights[12];       /* r_weights_ (R = diag(2r))                            */
  float mu;                  /* 0.3 (ConvexMpc.cpp:9)                                */
  float fz_min, fz_max;      /* 0 / 180 (ConvexMpc.cpp:227-228)                      */
  /* ADMM settings: OSQP names and defaults */
  float rho, sigma, alpha, eps_abs, eps_rel;
  int32_t max_iter, check_termination, scaling, adaptive_rho, adaptive_rho_interval;
  float adaptive_rho_tolerance;
  int32_t warm_start;        /* 0: cold start every call                            */
                             /* 1: osqp_warm_start from the unscaled x|y in warm    */
                             /*    (B*32N floats, in/out)                           */
                             /* 2: persistent solver, the reference's member        */
                             /*    OsqpEigen::Solver (A1RobotControl.cpp:556-578):  */
                             /*    warm = B*QLOCO_SRBD_PERSIST_LEN(N) floats, zeroed */
                             /*    before the first call; see DESIGN.md §3          */
  int32_t polish;            /* must be 0: OSQP polishing is not implemented (the    */
                             /* reference leaves it off); 1 -> QLOCO_ERR_ARG         */
  int32_t literal_full_qp;   /* 0: the stance-only reduction (swing forces removed  */
                             /*    exactly; same optimum, fastest kernels)          */
                             /* 1: the reference's call as written: all 12N forces  */
                             /*    are ADMM variables, swing legs held by their     */
                             /*    fz in [fz_min*c, fz_max*c] = [0, 0] rows (OSQP   */
                             /*    equality rows, rho_eq = 1e3 rho), Ruiz over the  */
                             /*    full P and A (ConvexMpc.cpp:162-264,             */
                             /*    A1RobotControl.cpp:557-578); DESIGN.md §3e       */
  int32_t reserved[5];       /* zero, but for the debug bit reserved[0] & 1: the one-  */
                             /* wave literal kernel builds its G^-1 horizon tables  */
                             /* per instance although the spec has host tables       */
                             /* (qloco_srbd_lit_tables); both paths stay tested;     */
                             /* and reserved[1] > 0: the SIMD count the placement    */
                             /* state assumes instead of the device's (tests reach   */
                             /* qloco_srbd_solve_placed's path at small batches)     */
} qloco_srbd_spec;

/* Per-instance record of the persistent solver (spec.warm_start == 2),
 * floats, full index (variable 12k+3i+c, constraint row 20k+5i+r):
 *   [0,12N) scaled x  [12N,32N) scaled z  [32N,52N) scaled y
 *   [52N,64N) unscaled x  [64N,84N) unscaled y  [84N,96N) unscaled q
 *   [96N,100N) contact flags  [100N] rho  [100N+1] 1 after the first call.
 * literal_full_qp = 1 (the reference's semantics): the first call sets the
 * solver up, EVERY later call takes OSQP's update path (osqp_update_P /
 * _lin_cost / _lower_bound / _upper_bound + solve: Ruiz on the new P with
 * the previous q in the cost scale, the rho vector re-typed from the new
 * bounds, the adapted rho kept, the scaled x, z, y carried) -- the
 * reference's Hessian pattern does not depend on the contacts, so OsqpEigen
 * never re-initialises.  literal_full_qp = 0 (stance-only reduction, whose
 * variable set follows the stance set): same stance set as the last call ->
 * the update path; a changed stance set re-initialises (settings rho),
 * warm-started from the last unscaled solution -- a documented deviation
 * from the reference. */
#define QLOCO_SRBD_PERSIST_LEN(N) (100 * (N) + 4)

/* Go1 SRBD constants + OSQP default settings. */
void qloco_srbd_spec_default(qloco_srbd_spec *spec);

/* Host-side G^-1 horizon tables of the literal QP's wrench-space kernels
 * (DESIGN.md §3l): a function of (horizon, dt, q_weights) alone where
 * q_weights[6] == q_weights[7] (isotropic omega x / y weights), computed once
 * per spec and passed to the one-wave kernel (horizon <= 10) with its
 * arguments.  gtab[gtab_len >= NT * NT * 6], NT = 10 for horizon <= 10 and 20
 * up to 20: (row step, column step, axis) in the kernels' column-space order
 * (two waves: step r >= H = ceil(N / 2) at 10 + r - H), float32 of the
 * float64 inverses of alpha_a K0 + beta_a K2, zero on padding steps.
 * *s_scale = 1 / sqrt(2 q_weights[6]), *gmx = max diag G^-1.  *served = 0 and
 * nothing else written where the kernels build the tables per instance
 * (anisotropic omega weights).  Host pointers; no device work. */
int qloco_srbd_lit_tables(const qloco_srbd_spec *spec, float *gtab, int64_t gtab_len,
                          float *s_scale, float *gmx, int32_t *served);

/* Largest stance-variable count the compiled kernels accept (3 x 4 x 20). */
int qloco_srbd_max_stance_vars(void);

/* Batched build + ADMM solve (the hot path).  Device pointers:
 *   x0[B*13]        mpc_states: [rpy, p, omega, v, -9.8]   (A1RobotControl.cpp:459-463)
 *   x_ref[B*13N]    mpc_states_d                             (:480-497)
 *   feet[B*12] or [B*12N]  foot_pos_abs, 3 per leg (FL,FR,RL,RR)
 *   contacts[B*4] or [B*4N] uint8 0/1
 * Outputs (NULL = not wanted, except u0):
 *   u0[B*12]        first-step forces (frame per spec->output_frame)
 *   u[B*12N]        full solution (world frame)
 *   status[B], iters[B] (ADMM iterations), obj[B] (QP objective)
 *   warm[B*(12N+20N)] in/out x|y warm-start state when spec->warm_start. */
int qloco_srbd_solve(const qloco_srbd_spec *spec, int64_t batch, const float *x0,
                     const float *x_ref, const float *feet, const uint8_t *contacts,
                     float *u0, float *u, int32_t *status, int32_t *iters, float *obj,
                     float *warm, void *stream);

/* Extended form of qloco_srbd_solve: additionally returns rho_updates[B]
 * (number of adaptive-rho refactorisations) and takes max_stance_legs, the
 * largest number of stance (step, leg) pairs of any instance in the batch,
 * or 0 = unknown (assume 4N).  Instances run by class: <= 21 stance pairs
 * in one-wavefront workgroups, 22..42 in two-wavefront workgroups, 43..80
 * (up to N = 20 all-stance, 240 variables) in the wide 512-thread kernel --
 * one launch per class the maximum admits, on the stream.  Any N <= 20
 * schedule is accepted; an instance with more stance pairs than a
 * caller-supplied max_stance_legs admits gets status QLOCO_BAD_SIZE, NaN u0 /
 * u / obj and iters = 0. */
int qloco_srbd_solve_ex(const qloco_srbd_spec *spec, int64_t batch, const float *x0,
                        const float *x_ref, const float *feet, const uint8_t *contacts,
                        float *u0, float *u, int32_t *status, int32_t *iters,
                        int32_t *rho_updates, float *obj, float *warm,
                        int32_t max_stance_legs, void *stream);

/* qloco_srbd_solve_ex with a placement state: `place`, device memory of
 * qloco_srbd_place_bytes(batch) bytes that the caller owns, zeroes once and
 * passes to every call of one controller batch (NULL = qloco_srbd_solve_ex).
 * A cold one-wave literal launch ends with its most loaded SIMD (DESIGN.md
 * §3q), so each call leaves every instance's iteration count in the state
 * and a small kernel after the solve, on the same stream, orders the next
 * call: the longest instances one per SIMD, the others dealt to them as
 * companions by rank: short ones to the long heads, one long,
 * one middle and one short to the rest.  Only which workgroup solves an
 * instance changes: every
 * output array is byte-identical to a call without the state, whatever the
 * state holds, and a controller whose counts drift or jump only loses the
 * gain.  The state is int32 words: a 4-word header (word 0 = batch once the
 * order is valid), hint[batch], order[batch]; all zero = no order yet.
 * It is used where QLOCO_ROUTE_LIT_ONE_WAVE runs with warm_start = 0 and
 * S < batch <= 4 S, S = 4 x the device's compute units (the batch resident at
 * once, more than one wave per SIMD); every other call ignores the pointer.
 * One stream at a time per state, as for the persistent record: calls that
 * share a state must be ordered on the device.  Write nothing into a state
 * but zeros. */
int64_t qloco_srbd_place_bytes(int64_t batch);
int qloco_srbd_solve_placed(const qloco_srbd_spec *spec, int64_t batch, const float *x0,
                            const float *x_ref, const float *feet, const uint8_t *contacts,
                            float *u0, float *u, int32_t *status, int32_t *iters,
                            int32_t *rho_updates, float *obj, float *warm,
                            int32_t max_stance_legs, int32_t *place, void *stream);

/* Per-instance body of the SRBD MPC: the five quantities of qloco_srbd_spec
 * that describe the robot rather than the problem, one 64-byte row per
 * instance.  A batch is a fleet: payload and friction randomised per robot,
 * A1 and Go1 bodies mixed (a yaml per robot becomes a row per robot). */
typedef struct qloco_srbd_model {
  float mass;
  float inertia[9];          /* col-major, as qloco_srbd_spec.inertia */
  float mu, fz_min, fz_max;
  float reserved[3];         /* zero */
} qloco_srbd_model;

/* rows[count] filled from the spec's mass, inertia, mu, fz_min and fz_max
 * (reserved zero): start from the defaults, edit a few rows.  Host pointers,
 * no device work. */
int qloco_srbd_model_from_spec(const qloco_srbd_spec *spec, int64_t count, qloco_srbd_model *rows);

/* qloco_srbd_solve_placed with per-instance bodies: `model` is device memory,
 * batch rows, or NULL.  NULL is exactly qloco_srbd_solve_placed (which, like
 * qloco_srbd_solve and _solve_ex, forwards here with NULL).  With rows,
 * instance b takes mass, inertia, mu, fz_min and fz_max from model[b] and
 * everything else from the spec; the spec's own five fields are then ignored,
 * except that they are validated as before.  The rows are read during the
 * call only and never written.
 *   Kernels: every family a call can take honours the rows -- the one-wave
 * literal kernel with and without the placement state (the row goes by the
 * instance id, not by the workgroup that solves it), the two-wave literal
 * kernel, the generic literal kernels, the reduced one- and two-wave classes
 * and the wide kernel (the row goes by the instance id the class list holds,
 * not by the position in the list).  The arithmetic is the uniform call's: an
 * instance's outputs are byte-identical to those of a call without rows whose
 * spec carries that row's values.  The route, the host G^-1 tables, the
 * placement state and the persistent record's layout do not depend on the
 * five quantities, and stay per batch; so do the weights and dt (they enter
 * the tables and the route).
 *   Warm start and the persistent solver: a controller's row may change
 * between calls.  With literal_full_qp = 1 every call after the first already
 * takes OSQP's update path with a new P, so nothing else happens.  With
 * literal_full_qp = 0 the existing rule holds: the record re-initialises only
 * when the stance set changes, a changed row alone takes the update path.
 *   An invalid row -- one of its 13 values not finite, or mass <= 0 -- is not
 * solved: that instance gets status QLOCO_ERR_ARG, NaN u0 / u / obj and
 * iters = rho_updates = 0 (as QLOCO_BAD_SIZE does for its case), its warm /
 * persistent record is left as it was, and every other instance of the batch
 * is unaffected.  QLOCO_ERR_ARG is otherwise a call-level code. */
int qloco_srbd_solve_model(const qloco_srbd_spec *spec, int64_t batch, const float *x0,
                           const float *x_ref, const float *feet, const uint8_t *contacts,
                           float *u0, float *u, int32_t *status, int32_t *iters,
                           int32_t *rho_updates, float *obj, float *warm,
                           int32_t max_stance_legs, int32_t *place,
                           const qloco_srbd_model *model, void *stream);

/* The ordering kernel's arithmetic on the host (tests): order[batch] from
 * hint[batch] for `simds` SIMDs, simds < batch <= 4 simds.  Instances by class
 * min(hint / max(check_termination, 1), 255), clamped at 0, the highest class
 * first; position s + simds q holds rank s for q = 0 and, from the short end,
 * SIMD s's q-th companion otherwise.  Any hint[] gives a permutation.  Host
 * pointers; QLOCO_ERR_ARG outside that range. */
int qloco_srbd_place_order_host(int64_t batch, int64_t simds, int32_t check_termination,
                                const int32_t *hint, int32_t *order);

/* The solve kernel's choice of rank on the host (tests, tools):
 * rank_of_position[p], p = s + simds q, is the rank (0 = longest) of the
 * instance that workgroup p solves, taken from order[] at that rank's
 * position.  A permutation of [0, batch) with rank s at q = 0.  Host pointer;
 * the refusals of qloco_srbd_place_order_host. */
int qloco_srbd_place_assign_host(int64_t batch, int64_t simds, int32_t *rank_of_position);

/* The kernel family a qloco_srbd_solve[_ex] call with this spec runs
 * (host-only, no device work; the solve uses the same decision):
 *   QLOCO_ROUTE_LIT_ONE_WAVE  literal QP, N <= 10: srbd_lit_kernel (one wavefront
 *                             per instance, the OSQP solve through the wrench space)
 *   QLOCO_ROUTE_LIT_TWO_WAVE  literal QP, N = 11..20: srbd_lit2_kernel
 *   QLOCO_ROUTE_LIT_GENERIC   literal QP otherwise (a q_omega / q_v weight of 0,
 *                             a state weight above 1000, per-step feet, N > 20):
 *                             the 12N-variable kernels
 *   QLOCO_ROUTE_REDUCED       literal_full_qp = 0: the stance-only classes
 * The Go1 defaults and the reference's config/{gazebo,hardware}_a1_mpc.yaml
 * sets take the wrench-space kernels, and so would anisotropic omega
 * weights of that size; config/isaac_a1_mpc.yaml's (roll 8000) take the
 * generic ones, where float32 converges as float64 does (the wrench-space
 * solve's precision limit).  Returns QLOCO_ERR_ARG on a bad
 * spec. */
#define QLOCO_ROUTE_LIT_ONE_WAVE 1
#define QLOCO_ROUTE_LIT_TWO_WAVE 2
#define QLOCO_ROUTE_LIT_GENERIC 3
#define QLOCO_ROUTE_REDUCED 4
int qloco_srbd_route(const qloco_srbd_spec *spec);

/* Class-dispatch scratch of qloco_srbd_solve_ex (instance lists, counters,
 * side streams, events): one set per (device, caller stream), at most 8
 * live -- the least recently used set beyond that is released.  Returns the
 * live sets; *pinned (may be NULL) = allocations kept for the life of the
 * process because a stream capture baked them into a graph. */
int qloco_srbd_scratch_sets(int32_t *pinned);

/* Batched condensed-QP build only (ConvexMpc::calculate_qp_mats, dense,
 * as the reference materialises it).  Outputs per instance (NULL = skip):
 *   H[B*(12N)^2] col-major, g[B*12N], lb[B*20N], ub[B*20N] (+-1e30 = INFTY),
 *   Aqp[B*13N*13], Bqp[B*13N*12N] col-major. */
int qloco_srbd_build(const qloco_srbd_spec *spec, int64_t batch, const float *x0,
                     const float *x_ref, const float *feet, const uint8_t *contacts,
                     float *H, float *g, float *lb, float *ub, float *Aqp, float *Bqp,
                     void *stream);
/* qloco_srbd_build with per-instance bodies (qloco_srbd_solve_model's rows:
 * device memory, batch rows, or NULL = qloco_srbd_build).  mu enters none of
 * these outputs.  The rows are not validated here: an invalid row gives what
 * its arithmetic gives. */
int qloco_srbd_build_model(const qloco_srbd_spec *spec, int64_t batch, const float *x0,
                           const float *x_ref, const float *feet, const uint8_t *contacts,
                           float *H, float *g, float *lb, float *ub, float *Aqp, float *Bqp,
                           const qloco_srbd_model *model, void *stream);

/* Deterministic synthetic instances, host memory.
 * gait: 0 trot, 1 pace (reference gait_mode 101), 2 mixed per-step, 3 stance.
 * x_ref must hold count*13N floats, contacts count*4N bytes. */
int qloco_gen_srbd_host(uint64_t seed, int32_t horizon, float dt, int32_t gait,
                        int64_t first, int64_t count, float *x0, float *x_ref,
                        float *feet, uint8_t *contacts);
/* Same instances for the global ids first + k * stride, k < count (the
 * interleaved shard of a rank: first = rank, stride = world). */
int qloco_gen_srbd_host_strided(uint64_t seed, int32_t horizon, float dt, int32_t gait,
                                int64_t first, int64_t stride, int64_t count, float *x0,
                                float *x_ref, float *feet, uint8_t *contacts);

/* ====================================================================== */
/* 2. Dense small-QP active-set solver (Goldfarb-Idnani), batched.          */
/*    replaces QPsolver_EiQuadProg::solve -> Eigen::QP::solve_quadprog      */
/*    (rt_mpc_qp/src/QP/QPBaseClass.cpp:36-58; EiQuadProg.cpp:172-513),     */
/*    quirk-compatible.  Double precision.              */
/*    n <= 64, p <= 64, m <= 320 (covers QPBaseClass's nVars <= 60,         */
/*    nIneq <= 300, QPBaseClass.h:49-51): n, p <= 16 and m <= 64 run four   */
/*    QPs per wavefront (bit-exact with the restatement in the common       */
/*    case), larger ones one per wavefront (to rounding; qloco_gi_wide.hip). */
/*    Matrices col-major, per instance:                                      */
/*    G[n*n] (only the lower triangle is read), g0[n], CE[n*p], ce0[p],     */
/*    CI[n*m], ci0[m].  A NULL CE/ce0/CI/ci0 with stride 0 broadcasts one    */
/*    shared copy; *_stride = elements between instances (0 = shared).     */
/*    Outputs x[B*n], f[B] (cost, +inf when infeasible), status[B],         */
/*    iters[B]; f, status and iters may be NULL.  QLOCO_NOT_PD stores        */
/*    x = 0, f = +inf, iters = 0.  More live (non-zero) CE columns than      */
/*    variables report QLOCO_DEGENERATE at column n + 1, x as the first n    */
/*    left it.                                                              */
/* ====================================================================== */
int qloco_eiquadprog_solve(int32_t n, int32_t p, int32_t m, int64_t batch, const double *G,
                           int64_t G_stride, const double *g0, int64_t g0_stride,
                           const double *CE, int64_t CE_stride, const double *ce0,
                           int64_t ce0_stride, const double *CI, int64_t CI_stride,
                           const double *ci0, int64_t ci0_stride, double *x, double *f,
                           int32_t *status, int32_t *iters, void *stream);
/* the largest n of the fast path (four QPs per wavefront, bit-exact in the */
/* common case): 16 -- unchanged since round 1; sizes above it up to        */
/* qloco_gi_limits run one QP per wavefront                                 */
int qloco_max_gi_vars(void);
/* the fast path's limits n, p, m (16, 16, 64; any pointer may be NULL)    */
void qloco_gi_fast_limits(int32_t *n, int32_t *p, int32_t *m);
/* the size limits above (QPBaseClass's capacity rounded up): n, p, m      */
/* (64, 64, 320; any pointer may be NULL)                                   */
void qloco_gi_limits(int32_t *n, int32_t *p, int32_t *m);

/* ====================================================================== */
/* 3. Go1 force-distribution QP, batched                                    */
/*    replaces Dynamiccclass::force_distribution + force_opt               */
/*    (go1_rt_control/src/whole_body_dynamics/dynmics_compute.cpp:141-373, */
/*    called at servo.cpp:1224-1228 and torque_mode.cpp:1364-1367)          */
/* ====================================================================== */
typedef struct qloco_force_params {
  double mass;    /* 12    dynmics_compute.cpp:31.  Stored and, as in Dynamiccclass, read by
                   * no kernel: without body rows F_sum is built with gait::mass = 12
                   * whatever stands here; a qloco_force_body row carries it into F_sum */
  double alpha;   /* 1e4   :61 */
  double beta;    /* 1e3   :62 */
  double gamma;   /* 10    :63 */
  double fz_max;  /* 160   :64 */
  double mu;      /* 0.25 sim (:65), 0.5 HW copy */
} qloco_force_params;
void qloco_force_params_default(qloco_force_params *p);

/* One robot's body for the Go1 force QP, the servo force block (section 7) and
 * the servo tick (section 16): the six qloco_force_params in the same order,
 * then the centroidal inertia Momentum_sum of servo.cpp:375-377.  The reference
 * has one Dynamiccclass and one gait::mass per process, so a fleet with
 * randomised payload, friction, force limits or gains is a row per robot here. */
typedef struct qloco_force_body {   /* 128 bytes */
  double mass, alpha, beta, gamma, fz_max, mu;
  double momentum[9];   /* Momentum_sum, row-major */
  double reserved[1];   /* zero */
} qloco_force_body;
/* rows[0 .. count) <- p's six fields and the reference's Momentum_sum (the same
 * nine expressions the kernels' constant is initialised with).  Host pointers,
 * no device work.  QLOCO_ERR_ARG for a NULL p, a negative count, or NULL rows
 * with count > 0. */
int qloco_force_body_from_params(const qloco_force_params *p, int64_t count,
                                 qloco_force_body *rows);
/* The row rule, on a host row: every field finite, mass > 0, alpha, beta,
 * gamma >= 0, fz_max >= 0, mu >= 0, reserved == 0.  alpha = beta = gamma = 0
 * passes (it solves to QLOCO_NOT_PD as it does per call).  QLOCO_OK or
 * QLOCO_ERR_ARG.  The kernels apply the same function to every row.  The
 * per-call qloco_force_params are not checked. */
int qloco_force_body_check(const qloco_force_body *row);

/* Per-instance inputs (device, double):
 *   com_des[B*3], leg_des[B*12], F_force_des[B*6], rfoot_des[B*3],
 *   lfoot_des[B*3]      -> force_distribution arguments
 *   base_p[B*3], feet_p[B*12] (FR,FL,RR,RL), FT_total_des[B*6] -> force_opt
 *   mode[B], right_support[B] (int32), y_coef[B]
 * Per-instance state (in/out, double): F_leg_ref[B*12] (3x4 col-major),
 *   grf_opt[B*12] (previous solution = F_prev of q_goal, :305).
 * Outputs: F_leg_guess[B*12], qp_solution[B] (int32, 1 = no NaN),
 *   status[B] (EiQuadProg outcome), iters[B].
 * qp_solution 0 (a NaN in the solution: status stays QLOCO_OK) stores
 *   grf_opt = F_leg_guess (:364-367).
 * Failed factorisation (status QLOCO_NOT_PD, iters 0: a non-positive or NaN
 *   Cholesky pivot, e.g. a NaN or Inf base_p[0] or foot x, or alpha = beta =
 *   gamma = 0): as in the reference, where solve_quadprog returns before it
 *   touches _X = grf_opt (:386-392, :437-443, EiQuadProg.cpp:505-510),
 *   grf_opt keeps its value from before the call, bit for bit, and
 *   qp_solution is 1 unless that carried vector holds a NaN (then grf_opt =
 *   F_leg_guess as above).  Unlike qloco_eiquadprog_solve, no x = 0 here.
 *   Departure from Eigen: a NaN pivot counts as failed (!(pivot > 0)); Eigen's
 *   LLT would run on to a NaN solution and the F_leg_guess fallback. */
int qloco_force_qp_solve(const qloco_force_params *prm, int64_t batch, const double *com_des,
                         const double *leg_des, const double *F_force_des,
                         const double *rfoot_des, const double *lfoot_des,
                         const double *base_p, const double *feet_p,
                         const double *FT_total_des, const int32_t *mode,
                         const int32_t *right_support, const double *y_coef,
                         double *F_leg_ref, double *grf_opt, double *F_leg_guess,
                         int32_t *qp_solution, int32_t *status, int32_t *iters,
                         void *stream);

/* The same solve with the robots grouped by control flow before the launch
 * (swing-leg pattern, then the robot's previous active-set iteration count):
 * the four robots that share a wavefront then take the same path.  Results
 * are bit-identical to qloco_force_qp_solve.  order_ws: device int32
 * workspace of qloco_force_order_ws_len(batch) entries, allocated and
 * zero-filled once by the caller and passed unchanged on every call -- like
 * F_leg_ref / grf_opt it carries per-robot state between calls (the
 * iteration counts that predict the next call's grouping); NULL = the
 * ungrouped launch.  No allocation happens inside, so the call can be
 * captured in a HIP graph. */
int64_t qloco_force_order_ws_len(int64_t batch);
int qloco_force_qp_solve_ordered(const qloco_force_params *prm, int64_t batch,
                                 const double *com_des, const double *leg_des,
                                 const double *F_force_des, const double *rfoot_des,
                                 const double *lfoot_des, const double *base_p,
                                 const double *feet_p, const double *FT_total_des,
                                 const int32_t *mode, const int32_t *right_support,
                                 const double *y_coef, double *F_leg_ref, double *grf_opt,
                                 double *F_leg_guess, int32_t *qp_solution, int32_t *status,
                                 int32_t *iters, int32_t *order_ws, void *stream);

/* qloco_force_qp_solve_ordered with per-robot bodies.  body: device memory,
 * `batch` rows, only read (`list` indexes them like every per-robot array); or
 * NULL, which is exactly qloco_force_qp_solve_ordered (it and
 * qloco_force_qp_solve forward here).  order_ws may be NULL as there.  With
 * rows, robot b builds G and g0 with body[b]'s alpha, beta, gamma and CI / ci0
 * with its mu, fz_max; mass and momentum are checked and not read; prm's
 * fields are then used only as the stand-in below.  A robot's outputs are
 * byte-identical to a call without rows whose prm carries its row's values,
 * whatever its position, group width, grouping or neighbours.
 *
 * A row qloco_force_body_check refuses is found on the device and refuses that
 * robot alone: status[b] = QLOCO_ERR_ARG, qp_solution[b] = 0, iters[b] = 0,
 * F_leg_guess NaN; F_leg_ref, grf_opt and the robot's iteration count in
 * order_ws keep their values bit for bit, so a robot whose row is corrected
 * continues from where it stood.  Its lanes run the solve with prm as a
 * stand-in, so its wavefront neighbours are byte-identical.  The call still
 * returns QLOCO_OK.  No allocation inside; capturable in a HIP graph (a linear
 * chain of nodes). */
int qloco_force_qp_solve_body(const qloco_force_params *prm, int64_t batch,
                              const double *com_des, const double *leg_des,
                              const double *F_force_des, const double *rfoot_des,
                              const double *lfoot_des, const double *base_p,
                              const double *feet_p, const double *FT_total_des,
                              const int32_t *mode, const int32_t *right_support,
                              const double *y_coef, double *F_leg_ref, double *grf_opt,
                              double *F_leg_guess, int32_t *qp_solution, int32_t *status,
                              int32_t *iters, int32_t *order_ws,
                              const qloco_force_body *body, void *stream);

/* The hardware servo's Dynamiccclass constants (unitree_legged_real copy of
 * dynmics_compute.cpp:31,65: mass = gait::mass = 14, robot_const_para_config
 * .cpp:28; mu = 0.5), the call at torque_mode.cpp:1364-1367; the other
 * fields as qloco_force_params_default (the sim copy: mass 12, mu 0.25). */
void qloco_force_params_hw(qloco_force_params *p);

/* Robots per wavefront of the force-QP kernel: 8 (eight 8-lane groups, the
 * default) or 16 (four 16-lane groups).  The outputs are bit-identical
 * either way; the knob exists for A/B measurements and the test that pins
 * that identity (QLOCO_FORCE_GW=16 in the environment sets the initial
 * value).  Returns the previous width, or QLOCO_ERR_ARG for other values.
 * Process-wide; set it while no force-QP launch is being enqueued. */
int qloco_force_set_group_width(int gw);

/* The hardware loop's feed-forward after force_opt (unitree_legged_real
 * torque_mode.cpp:1370-1384): rate = min((dynamic_count / 500)^2, 1),
 * F_opt = rate (grf_opt - grf_base) + grf_base per leg (grf_base: the
 * stand-up FR_GRF .. RL_GRF of :1057-1058), tau = -J^T F_opt -- no gravity
 * compensation.  Per instance: Jaco[4*9] (col-major per leg), grf_opt[12],
 * grf_base[12], dynamic_count (int32) -> tau[12]; legs FR, FL, RR, RL. */
int qloco_hw_torque_ff(int64_t batch, const double *Jaco, const double *grf_opt,
                       const double *grf_base, const int32_t *dynamic_count, double *tau,
                       void *stream);

/* Joint torques tau = -J^T F + g_comp (stance) or PD (swing),
 * Dynamiccclass::compute_joint_torques (dynmics_compute.cpp:109-138), for
 * all 4 legs of B instances.  Jaco[B*4*9] col-major per leg, swing[B*4],
 * p_des/p_est/pv_des/pv_est[B*12], F_leg_ref[B*12] -> tau[B*12]. */
int qloco_joint_torques(int64_t batch, const double *Jaco, const int32_t *swing,
                        const double *p_des, const double *p_est, const double *pv_des,
                        const double *pv_est, const double *F_leg_ref, double *tau,
                        void *stream);

/* ====================================================================== */
/* 4. rt body-inclination MPC step, batched                                 */
/*    replaces PRMPCClass::body_theta_mpc (rt_mpc_qp/src/FastMPC/          */
/*    PRMPCClass.cpp:379-714) called at gait_fast.cpp:620                  */
/* ====================================================================== */
/* Per-instance state record (double[32]), created by qloco_body_state_init:
 *   [0:2] thetaxk  [2:4] thetayk  [4:12] V_ini  [12:26] last com_traj
 *   [26] bjx1 [27] bjx2 [28] t_yu [29] qp_solution [30:32] reserved        */
#define QLOCO_BODY_STATE_LEN 32
int qloco_body_state_init_host(int64_t batch, double *state);
/* i[B] (loop counter, int32), bodyangle_state[B*4], zmp_ref/angle_ref/
 * rfoot_ref/lfoot_ref[B*10] (Eigen 2x5 col-major), comacc_ref[B*15] (3x5)
 * -> com_traj[B*14]; state in/out; status[B] EiQuadProg outcome.
 * QLOCO_NOT_PD: G is positive definite for finite inputs (constants plus
 * (j_ini / (mass (comacc_z + g)))^2 >= 0 on the diagonal), so only a NaN
 * comacc_ref z in the horizon fails, through the NaN-pivot rule of section
 * 3.  _X = _V_ini then stays as it was before the call, which is what the
 * reference's failed solve leaves (:803, :843-847), and the post-processing
 * runs on it. */
int qloco_body_mpc_step(int64_t batch, const int32_t *i, const double *bodyangle_state,
                        const double *zmp_ref, const double *angle_ref,
                        const double *rfoot_ref, const double *lfoot_ref,
                        const double *comacc_ref, double *state, double *com_traj,
                        int32_t *status, void *stream);
/* PRMPCClass::Indexfind (PRMPCClass.cpp:716-738) on B fp64 times -> int32 */
int qloco_body_indexfind(int64_t batch, const double *t, int32_t *j_period, void *stream);

/* ====================================================================== */
/* 5. Go1 leg kinematics, batched (fp64, one leg per lane)                  */
/*    replaces Kinematicclass (go1_rt_control/src/kinematics/Kinematics.cpp) */
/*    called per leg at servo.cpp:734-741 (FK_g + Jacobian_kin) and         */
/*    servo.cpp:1038-1051 (IK_g + Jacobian_kin)                             */
/* ====================================================================== */
/* Forward_kinematics (:63-142, body_p = body_r = NULL: hip frame) or
 * Forward_kinematics_g (:145-229; body_p[n*3], body_r[n*3] = roll, pitch,
 * yaw).  q[n*3] (hip, thigh, calf), leg[n] (0 FR, 1 FL, 2 RR, 3 RL)
 * -> pos[n*3], jac[n*9] (Jacobian_kin, 3x3 column-major; may be NULL). */
int qloco_leg_fk(int64_t n, const double *q, const int32_t *leg, const double *body_p,
                 const double *body_r, double *pos, double *jac, void *stream);
/* Inverse_kinematics (:233-267, 10 damped Newton steps, lamda 0.5) or
 * Inverse_kinematics_g (:270-304, 15 steps) from q_ini[n*3] toward
 * pos_des[n*3] -> q_out[n*3]; optional pos[n*3] / jac[n*9] at q_out (the
 * reference's pos_cal / Jacobian_kin after the call) and updates[n] (Newton
 * steps applied).  Reference stop tests reproduced as written. */
int qloco_leg_ik(int64_t n, const double *pos_des, const double *q_ini, const int32_t *leg,
                 const double *body_p, const double *body_r, double *q_out, double *pos,
                 double *jac, int32_t *updates, void *stream);

/* ====================================================================== */
/* 6. rt_mpc_qp node tick, batched                 */
/*    replaces one iteration of the rt node loop, unitree_ros/rt_mpc_qp/   */
/*    src/gait_fast.cpp:505-735: callbacks (:79-110), counters and         */
/*    /rt2nrt/state (:512-527), xget_position_interpolation (:113-372 ->   */
/*    PRMPCClass::XGetSolution_position_mod3, PRMPCClass.cpp:1170-1261),   */
/*    Foot_trajectory_solve_mod2 (:1756-2195) + Indexfind (:716-738),      */
/*    XGetSolution_Foot_rotation (:2255-2380), body_theta_mpc (:379-714)   */
/*    and the /rtMPC/traj message (gait_fast.cpp:633-729)                  */
/* ====================================================================== */
/* Wire formats, one message per robot, row-major [B][len], double:
 *   /MPC/Gait            gait_msg[B*100]  (NLPRTControlClass.cpp:284-392;
 *                        [86..94] = Nrtfoorpr_gen, [99] = mpc_gait_flag)
 *   /control2rtmpc/state ctrl_msg[B*25]   ([0] > 0 starts the loop; [10],
 *                        [11], [13], [14] = bodyangle_state, gait_fast.cpp:105-108)
 *   /rtMPC/traj          traj_msg[B*100]  ([0..35] = gait_msg[0..35],
 *                        [36..86] = low_mpc_gait_inte, [86] = 0 (the node's
 *                        wall-clock duration), [98] = (int)_tx_total/0.001,
 *                        [99] = count_in_rt_loop)
 *   /rt2nrt/state        nrt_msg[B*25]    (last published state_to_MPC)  */
#define QLOCO_GAIT_MSG_LEN 100
#define QLOCO_CTRL_MSG_LEN 25
#define QLOCO_TRAJ_MSG_LEN 100
#define QLOCO_NRT_MSG_LEN 25
/* sched[B*8] (optional): bjx1, bjxx, t_end_footstep, count_in_rt_mpc, t_int,
 * body EiQuadProg status (-1 = body_theta_mpc not called this tick),
 * /rt2nrt/state published this tick (0/1), bjx2 */
#define QLOCO_RT_SCHED_LEN 8
/* Bytes of the device workspace holding B robots' node + PRMPCClass state. */
int64_t qloco_rt_workspace_bytes(int64_t batch);
/* PRMPCClass() + Initialize() + gait_fast.cpp main() init (:384-502) for B
 * robots, on device. */
int qloco_rt_init(int64_t batch, void *workspace, void *stream);
/* One loop iteration for B robots, given each robot's latest /MPC/Gait and
 * /control2rtmpc/state (device pointers).  gen[B*60] (optional) =
 * foorpr_gen (30) | foortheta_gen (30). */
int qloco_rt_tick(int64_t batch, void *workspace, const double *gait_msg,
                  const double *ctrl_msg, double *traj_msg, double *nrt_msg, double *gen,
                  int32_t *sched, void *stream);

/* ====================================================================== */
/* 7. go1 servo force block, batched                */
/*    replaces servo.cpp:1052-1243 (+ :1318) of go1_rt_control: leg        */
/*    positions, body-relative desired feet and their velocity, F_sum,      */
/*    rleg_com / F_lr_predict, swing flags, then Dynamiccclass::            */
/*    force_distribution + force_opt and compute_joint_torques x 4          */
/* ====================================================================== */
/* Per-robot inputs (device, double unless noted), legs FR, FL, RR, RL:
 *   coma_des[B*3], com_des[B*3], rfoot_des[B*3], lfoot_des[B*3],
 *   body_p_des[B*3], foot_des[B*12] (desired feet, world frame),
 *   right_support[B], gait_mode[B], loop_count[B] (int32; count_in_rt_loop),
 *   y_offset[B], Jaco[B*4*9] (each leg's 3x3 Jacobian_kin, col-major),
 *   foot_rel_mea[B*12] (measured foot - body), v_est_rel[B*12].
 * Outputs: grf_opt[B*12] and tau[B*12] (Legs_torque) required; F_sum[B*6],
 *   Force_L_R[B*6] (F_lr_predict), swing[B*4], qp_solution[B], status[B]
 *   optional.  Member / loop state (F_leg_ref, grf_opt, swing flags,
 *   relative_des_old, v_relative) lives in the workspace. */
int64_t qloco_servo_workspace_bytes(int64_t batch);
int qloco_servo_init(int64_t batch, void *workspace, void *stream);
int qloco_servo_force_block(const qloco_force_params *prm, int64_t batch, void *workspace,
                            const double *coma_des, const double *com_des,
                            const double *rfoot_des, const double *lfoot_des,
                            const double *body_p_des, const double *foot_des,
                            const int32_t *right_support, const int32_t *gait_mode,
                            const double *y_offset, const int32_t *loop_count,
                            const double *Jaco, const double *foot_rel_mea,
                            const double *v_est_rel, double *F_sum, double *Force_L_R,
                            double *grf_opt, double *tau, int32_t *swing,
                            int32_t *qp_solution, int32_t *status, void *stream);
/* The force block with per-robot bodies (section 3's qloco_force_body; device,
 * `batch` rows, or NULL = qloco_servo_force_block, which forwards here).  With
 * rows, F_sum of robot b is mass*ca[0], mass*ca[1], mass*g + mass*ca[2],
 * momentum . ca with its row's mass and momentum, in the operation order of
 * the call without rows (a row holding 12 and Momentum_sum is byte-identical
 * to NULL), and the force QP takes the row as qloco_force_qp_solve_body does.
 * A refused row: the glue computes F_sum with the constants as a stand-in,
 * the QP refuses the robot (status QLOCO_ERR_ARG, qp_solution 0; F_leg_ref and
 * grf_opt in the workspace unchanged, nothing non-finite enters the
 * workspace), and the caller's tau and grf_opt rows of that robot are NaN. */
int qloco_servo_force_block_body(const qloco_force_params *prm, int64_t batch, void *workspace,
                                 const double *coma_des, const double *com_des,
                                 const double *rfoot_des, const double *lfoot_des,
                                 const double *body_p_des, const double *foot_des,
                                 const int32_t *right_support, const int32_t *gait_mode,
                                 const double *y_offset, const int32_t *loop_count,
                                 const double *Jaco, const double *foot_rel_mea,
                                 const double *v_est_rel, double *F_sum, double *Force_L_R,
                                 double *grf_opt, double *tau, int32_t *swing,
                                 int32_t *qp_solution, int32_t *status,
                                 const qloco_force_body *body, void *stream);

/* ====================================================================== */
/* 8. slow planner's contact-phase flag, batched     */
/*    replaces the schedule indices of NLPClass::step_timing_opti_loop     */
/*    (mosek_nlp_kmp NLPClass_sqp.cpp:1029-1039) and the right_support     */
/*    branch of NLPClass::Foot_trajectory_solve_mod2 (:2076-2090,          */
/*    :2187-2202, :2311-2313) -- the /MPC/Gait[99] flag servo.cpp:673 reads */
/* ====================================================================== */
/* ts[B*27], tx[B*27] (device, double): each robot's _ts / _tx after the
 * planner's step-timing update (row per robot); t_int[B] (_t_int, the slow
 * loop index) and t_end_footstep[B] (int32).  Outputs (int32): bjxx[B] and
 * bjx1[B] (optional), right_support[B] (0 left, 1 right, 2 double
 * support).  Integer results are bit-exact with the restatement. */
#define QLOCO_NLP_STEPS 27
int qloco_support_phase(int64_t batch, const double *ts, const double *tx, const int32_t *t_int,
                        const int32_t *t_end_footstep, int32_t *bjxx, int32_t *bjx1,
                        int32_t *right_support, void *stream);

/* ====================================================================== */
/* 9. A1 single-step force QP, batched (fp64)                               */
/*    replaces the stance_leg_control_type == 0 branch of                  */
/*    A1RobotControl::compute_grf (unitree_ros/a1_cpp_open_source/src/     */
/*    A1RobotControl.cpp:383-450; constructor :8-49): root_acc from PD      */
/*    gains, H = R I + inv' Q inv, g = -inv' Q root_acc, 20-row friction    */
/*    pyramid / normal-force block, cold OSQP solve with default settings,  */
/*    forces rotated into the body frame.                                   */
/* ====================================================================== */
typedef struct qloco_a1_params {
  double kp_linear[3], kd_linear[3], kp_angular[3], kd_angular[3]; /* A1CtrlStates.h:123-126 */
  double robot_mass;                                                /* A1CtrlStates.h:39 */
  double q_diag[6];  /* Q (A1RobotControl.cpp:12) */
  double r;          /* R = 1e-3 (:13) */
  double mu;         /* 0.7 (:14) */
  double f_min, f_max; /* 0 / 180 (:15-16) */
  /* OSQP settings (defaults = OsqpEigen's, i.e. OSQP v0.6 defaults) */
  double rho, sigma, alpha, eps_abs, eps_rel, adaptive_rho_tolerance;
  int32_t max_iter, check_termination, scaling, adaptive_rho, adaptive_rho_interval;
  int32_t reserved[3];
} qloco_a1_params;
void qloco_a1_params_default(qloco_a1_params *p);
/* The parameter rule.  QLOCO_OK, or QLOCO_ERR_ARG (qloco_last_error() names
 * the field) for what OSQP v0.6's validate_settings refuses -- max_iter < 1,
 * scaling < 0, check_termination < 0, adaptive_rho_interval < 0, rho <= 0,
 * sigma <= 0, alpha outside (0, 2), eps_abs < 0, eps_rel < 0, both zero,
 * adaptive_rho_tolerance < 1 -- and for a body the QP is not posed for: any
 * non-finite double field, robot_mass <= 0, mu < 0, f_min > f_max, r < 0, a
 * negative q_diag entry.  qloco_a1_qp_solve applies it before any device
 * work; check_termination = 0 is legal (no termination check: the solve runs
 * max_iter iterations and the adaptive-rho interval becomes 100). */
int qloco_a1_params_check(const qloco_a1_params *p);
/* Per-robot state record, double[QLOCO_A1_STATE_LEN] (A1CtrlStates fields):
 *   [0:3] root_pos  [3:6] root_pos_d  [6:9] root_euler  [9:12] root_euler_d
 *   [12:15] root_lin_vel (world)  [15:18] root_lin_vel_d (body)
 *   [18:21] root_ang_vel (world)  [21:24] root_ang_vel_d (body)
 *   [24:33] root_rot_mat  [33:42] root_rot_mat_z  (3x3 col-major)
 *   [42:54] foot_pos_abs (3x4 col-major, legs FL, FR, RL, RR)
 * contacts[B*4] uint8.  Outputs: forces_body[B*12] (foot_forces_grf, 3x4
 * col-major) required; qp_solution[B*12] (world frame), status[B],
 * iters[B], rho_updates[B], obj[B] optional (NULL); forces_body does not
 * depend on which of them are given.  A contact flag is set when its byte is
 * non-zero.
 *
 * Failed solves (per robot, status[b]; the call still returns QLOCO_OK):
 *   QLOCO_MAX_ITER / QLOCO_SOLVED_INACCURATE  the ADMM ran max_iter iterations
 *     without passing a termination check (iters[b] == max_iter); the status
 *     is SOLVED_INACCURATE if the last iterate passes the check at 10 x eps
 *     (OSQP's rule, evaluated at max_iter whether or not that is a check
 *     iteration), else MAX_ITER.  forces_body and qp_solution hold the last
 *     iterate, finite, as OSQP returns it.
 *   QLOCO_NAN  the objective of the last iterate is not finite (a NaN or Inf
 *     in the robot's state record): forces_body and qp_solution of that robot
 *     are NaN, iters[b] is where the loop stopped.  This is the kernel's own
 *     contract; OSQP would report a finite-looking status there.  Other robots
 *     of the batch are not affected: their outputs are bit-identical to a
 *     call in which that robot's record is finite. */
#define QLOCO_A1_STATE_LEN 54
int qloco_a1_qp_solve(const qloco_a1_params *prm, int64_t batch, const double *state,
                      const uint8_t *contacts, double *forces_body, double *qp_solution,
                      int32_t *status, int32_t *iters, int32_t *rho_updates, double *obj,
                      void *stream);
/* One robot's body and controller tuning: the first 23 doubles of
 * qloco_a1_params in the same order (everything up to `rho`), plus one pad.
 * The reference controller has one A1CtrlStates per process, so a fleet with
 * randomised payloads, friction or gains is a row per robot here where it is a
 * yaml per robot there.  The OSQP settings (rho .. adaptive_rho_interval) stay
 * per batch: they steer the trip counts and the shape of the loop. */
typedef struct qloco_a1_body {            /* 192 bytes */
  double kp_linear[3], kd_linear[3], kp_angular[3], kd_angular[3];
  double robot_mass;
  double q_diag[6];
  double r;
  double mu;
  double f_min, f_max;
  double reserved;                        /* written 0 by the helpers, not read */
} qloco_a1_body;
/* rows[0 .. count) <- the body fields of p (host pointers, no device work).
 * QLOCO_ERR_ARG for a NULL p, a negative count, or NULL rows with count > 0. */
int qloco_a1_body_from_params(const qloco_a1_params *p, int64_t count, qloco_a1_body *rows);
/* The body half of the parameter rule above, on a host row: every double
 * finite, robot_mass > 0, mu >= 0, f_min <= f_max, r >= 0, no negative q_diag
 * entry (`reserved` is not read).  QLOCO_OK, or QLOCO_ERR_ARG with the field
 * named by qloco_last_error().  It is the same function qloco_a1_params_check
 * applies to the parameters' body fields, and the one the kernel applies to
 * every row. */
int qloco_a1_body_check(const qloco_a1_body *row);
/* qloco_a1_qp_solve with per-robot bodies.  body: device memory, `batch`
 * rows, only read; or NULL, which is exactly qloco_a1_qp_solve (it forwards
 * here).  With rows, robot b takes the 23 body quantities from body[b] and
 * the solver settings from prm; prm's own body fields are then ignored,
 * except that prm is still validated whole before any device work.
 *
 * A robot's outputs are byte-identical to those of a call without rows whose
 * prm carries its row's values, whatever its position in the batch, its
 * neighbours' bodies and the optional outputs given.
 *
 * An invalid row (one qloco_a1_body_check refuses) is found on the device and
 * that robot is not solved: status[b] = QLOCO_ERR_ARG, forces_body,
 * qp_solution and obj NaN, iters[b] = rho_updates[b] = 0; the call still
 * returns QLOCO_OK and every other robot is bit-identical to a call in which
 * that row is valid.  QLOCO_ERR_ARG wins over QLOCO_NAN where both apply.
 *
 * Still one value per batch: the solver settings.  The Go1 force QP
 * (section 3) and the servo ticks (sections 7, 16) take qloco_force_body rows. */
int qloco_a1_qp_solve_body(const qloco_a1_params *prm, int64_t batch, const double *state,
                           const uint8_t *contacts, double *forces_body, double *qp_solution,
                           int32_t *status, int32_t *iters, int32_t *rho_updates, double *obj,
                           const qloco_a1_body *body, void *stream);

/* ====================================================================== */
/* 10. Multi-GPU handles                         */
/*    The instances are independent: each rank (one process or thread per */
/*    GPU) solves its own shard of the global batch with                   */
/*    qloco_srbd_solve_ex and ONE RCCL all-gather over xGMI, on the        */
/*    caller's stream, leaves every rank with u0 of the whole batch in     */
/*    global instance order.  Replaces nothing in the reference (its       */
/*    controllers are one process each, A1RobotControl.cpp:553-578); it is */
/*    the C++ caller's way to shard.  RCCL (librccl.so.1) is loaded on     */
/*    first use.                                                           */
/* ====================================================================== */
#define QLOCO_MGPU_ID_BYTES 128
enum {
  QLOCO_SHARD_CONTIGUOUS = 0,  /* balanced contiguous ranges                        */
  QLOCO_SHARD_INTERLEAVED = 1  /* ids rank, rank + world, ... (divergent schedules) */
};
typedef struct qloco_mgpu qloco_mgpu;
/* Global ids owned by `rank`: first + k * stride, k < count.  Contiguous:
 * first = rank * (total / world) + min(rank, total % world), count = total /
 * world (+1 for rank < total % world), stride 1.  Interleaved: first = rank,
 * stride = world, count = ceil((total - rank) / world).  Host only. */
int qloco_mgpu_shard(int64_t total, int32_t world, int32_t rank, int32_t mode, int64_t *first,
                     int64_t *count, int64_t *stride);
/* Row of global id g in the gathered (world x P) buffer, P = ceil(total /
 * world) the padded shard: rows[g] = owner * P + position.  Host only (the
 * device reorder uses the same map). */
int qloco_mgpu_gather_rows(int64_t total, int32_t world, int32_t mode, int64_t *rows);
/* The device half of qloco_mgpu_solve's step 3, for a caller that runs its
 * own all-gather (e.g. torch.distributed): `stage` holds the gathered
 * (world x P x width) shard rows, P = ceil(total / world), width 12 (u0) or
 * 14 (u0, then status and iterations as raw int32 bits); writes u0_all
 * [total*12] and, for width 14, status_all / iters_all [total] (optional) in
 * global id order -- the map of qloco_mgpu_gather_rows.  Device pointers,
 * stream-ordered on `stream`. */
int qloco_mgpu_reorder(int64_t total, int32_t world, int32_t mode, int32_t width, const float *stage,
                       float *u0_all, int32_t *status_all, int32_t *iters_all, void *stream);
/* Rank 0: a new communicator id; the caller ships the bytes to every rank. */
int qloco_mgpu_unique_id(uint8_t *id /* [QLOCO_MGPU_ID_BYTES] */);
/* Collective: every rank, with its device current, the same id / world /
 * total / mode.  Allocates the rank's padded shard buffers on that device. */
int qloco_mgpu_init(qloco_mgpu **h, const uint8_t *id, int32_t world, int32_t rank, int64_t total,
                    int32_t mode);
/* This rank's shard (first, count, stride) and the padded shard size P. */
int qloco_mgpu_info(const qloco_mgpu *h, int64_t *first, int64_t *count, int64_t *stride,
                    int64_t *padded);
/* Solve this rank's shard -- x0 / x_ref / feet / contacts / warm hold ITS
 * `count` instances, laid out as for qloco_srbd_solve_ex -- then all-gather:
 * u0_all[total*12] (required), status_all[total], iters_all[total]
 * (optional) in global id order on every rank.  Collective and stream-
 * ordered on `stream` (the handle's device must be current). */
int qloco_mgpu_solve(qloco_mgpu *h, const qloco_srbd_spec *spec, const float *x0,
                     const float *x_ref, const float *feet, const uint8_t *contacts, float *warm,
                     float *u0_all, int32_t *status_all, int32_t *iters_all,
                     int32_t max_stance_legs, void *stream);
/* qloco_mgpu_solve with per-instance bodies (qloco_srbd_solve_model): `model`
 * holds this rank's own `count` rows, in the order of its other shard inputs
 * (device memory), or NULL = qloco_mgpu_solve. */
int qloco_mgpu_solve_model(qloco_mgpu *h, const qloco_srbd_spec *spec, const float *x0,
                           const float *x_ref, const float *feet, const uint8_t *contacts,
                           float *warm, float *u0_all, int32_t *status_all, int32_t *iters_all,
                           int32_t max_stance_legs, const qloco_srbd_model *model, void *stream);
/* Releases the communicator and the buffers (NULL is a no-op). */
int qloco_mgpu_destroy(qloco_mgpu *h);

/* ====================================================================== */
/* 11. A1 leg kinematics, batched (fp64)                                   */
/*    replaces the per-leg block of GazeboA1ROS::gt_pose_callback          */
/*    (unitree_ros/a1_cpp_open_source/src/GazeboA1ROS.cpp:306-331):        */
/*    A1Kinematics::fk / jac (legKinematics/A1Kinematics.cpp:39-130),      */
/*    foot_vel_rel = J qdot, root_quat.toRotationMatrix(),                 */
/*    Utils::quat_to_euler (utils/Utils.cpp:7-33, asin clamp included),    */
/*    the yaw-only root_rot_mat_z and the body / world frame copies.       */
/* ====================================================================== */
typedef struct qloco_a1_kin_params {
  double rho_fix[4][5]; /* per leg: leg_offset_x, leg_offset_y, motor_offset, upper, lower */
                        /* (GazeboA1ROS.cpp:79-101)                                        */
  double rho_opt[4][3]; /* 0 (:98-99)                                                      */
} qloco_a1_kin_params;
void qloco_a1_kin_params_default(qloco_a1_kin_params *p);
/* Device pointers, double, legs FL, FR, RL, RR.  Inputs: joint_pos[B*12],
 * joint_vel[B*12], root_quat[B*4] as (w, x, y, z); root_pos[B*3] and
 * root_lin_vel[B*3] optional (needed by foot_pos_world / foot_vel_world).
 * Outputs, all optional (NULL) except foot_pos_rel: foot_pos_rel[B*12] (3x4
 * col-major), j_foot[B*36] (the four 3x3 diagonal blocks of j_foot, each
 * col-major), foot_vel_rel[B*12], root_rot_mat[B*9], root_euler[B*3],
 * root_rot_mat_z[B*9] (3x3 col-major), foot_pos_abs / foot_vel_abs /
 * foot_pos_world / foot_vel_world [B*12].  With a row stride of
 * QLOCO_A1_STATE_LEN the outputs are the [6:9], [24:33], [33:42] and [42:54]
 * fields of the section 9 record; this entry point writes dense arrays. */
int qloco_a1_leg_kin(const qloco_a1_kin_params *prm, int64_t batch, const double *joint_pos,
                     const double *joint_vel, const double *root_quat, const double *root_pos,
                     const double *root_lin_vel, double *foot_pos_rel, double *j_foot,
                     double *foot_vel_rel, double *root_rot_mat, double *root_euler,
                     double *root_rot_mat_z, double *foot_pos_abs, double *foot_vel_abs,
                     double *foot_pos_world, double *foot_vel_world, void *stream);

/* ====================================================================== */
/* 12. A1 state estimator, batched (fp64)                                  */
/*    replaces A1BasicEKF (unitree_ros/a1_cpp_open_source/src/             */
/*    A1BasicEKF.h:16-72, A1BasicEKF.cpp:7-164) as GazeboA1ROS::main_update */
/*    calls it (GazeboA1ROS.cpp:204-209): init_state on the first tick,     */
/*    update_estimation afterwards; 18 states (pos, vel, four feet), 28     */
/*    measurements.  S is factored once (Cholesky) where the reference      */
/*    solves twice with fullPivHouseholderQr; results agree to rounding.    */
/* ====================================================================== */
typedef struct qloco_a1_ekf_params {
  double process_noise_pimu, process_noise_vimu, process_noise_pfoot; /* A1BasicEKF.h:16-18 */
  double sensor_noise_pimu_rel_foot, sensor_noise_vimu_rel_foot;      /* :19-20 */
  double sensor_noise_zfoot;                                          /* :21 */
  int32_t assume_flat_ground; /* 1: the default-constructed member (GazeboA1ROS.h:160) */
  int32_t reserved[7];
} qloco_a1_ekf_params;
void qloco_a1_ekf_params_default(qloco_a1_ekf_params *p);
/* The filter state (x, P) of every robot lives in a device workspace of
 * qloco_a1_ekf_workspace_bytes(batch) bytes (-1 for batch <= 0):
 * QLOCO_A1_EKF_WS doubles per robot = x[18] | P, packed lower triangle, row
 * by row [171] | pad. */
#define QLOCO_A1_EKF_WS 192
#define QLOCO_A1_EKF_STATE 18
#define QLOCO_A1_EKF_MEAS 28
int64_t qloco_a1_ekf_workspace_bytes(int64_t batch);
/* init_state (A1BasicEKF.cpp:55-68): P = 3 I, x = (0, 0, 0.09, 0.., R fk_i + pos). */
int qloco_a1_ekf_init(const qloco_a1_ekf_params *prm, int64_t batch, void *workspace,
                      const double *root_rot_mat, const double *foot_pos_rel, void *stream);
/* update_estimation (A1BasicEKF.cpp:70-164), one tick of every robot.
 * Device pointers: dt[B], movement_mode[B] (int32), root_rot_mat[B*9] (3x3
 * col-major), imu_acc[B*3], imu_ang_vel[B*3], foot_pos_rel[B*12],
 * foot_vel_rel[B*12] (3x4 col-major), foot_force[B*4].  Outputs:
 * root_pos[B*3] = x[0:3] and root_lin_vel[B*3] = x[3:6] required;
 * estimated_contacts[B*4] (uint8) optional. */
int qloco_a1_ekf_update(const qloco_a1_ekf_params *prm, int64_t batch, void *workspace,
                        const double *dt, const int32_t *movement_mode,
                        const double *root_rot_mat, const double *imu_acc,
                        const double *imu_ang_vel, const double *foot_pos_rel,
                        const double *foot_vel_rel, const double *foot_force, double *root_pos,
                        double *root_lin_vel, uint8_t *estimated_contacts, void *stream);
/* Dense x[B*18] and P[B*324] (18x18 col-major) out of / into the workspace
 * (tests, logging, checkpoints).  set_state reads P's lower triangle. */
int qloco_a1_ekf_get_state(int64_t batch, const void *workspace, double *x, double *P,
                           void *stream);
int qloco_a1_ekf_set_state(int64_t batch, void *workspace, const double *x, const double *P,
                           void *stream);

/* ====================================================================== */
/* 13. A1 gait plan, swing-leg control, terrain pitch and joint torques,   */
/*    batched (fp64)                                                       */
/*    replaces A1RobotControl::update_plan + generate_swing_legs_ctrl      */
/*    (unitree_ros/a1_cpp_open_source/src/A1RobotControl.cpp:149-292, as    */
/*    GazeboA1ROS.cpp:199-202 calls them back to back), the                */
/*    stance_leg_control_type == 1 preamble of compute_grf (:341-380, with  */
/*    compute_walking_surface :604-620 and Utils.cpp:44-62) and             */
/*    compute_joint_torques (:294-324).  With sections 9 / 1, 11 and 12 one */
/*    A1 control tick runs on the device: leg kinematics, plan + swing,     */
/*    EKF, terrain pitch, QP or MPC, joint torques.                         */
/* ====================================================================== */
/* Defaults from A1CtrlStates::reset() (A1CtrlStates.h:20-132), A1Params.h:38-45
 * and the A1RobotControl constructor (:53-58).  a1_ctrl.launch's yaml
 * overrides several of them through resetFromROSParam (A1CtrlStates.h:134-317:
 * the gait counter speeds, default_foot_pos, kp_foot / kd_foot / km_foot among
 * others); a caller that runs with that yaml passes its values here.  3x4
 * matrices are column-major, legs FL, FR, RL, RR. */
typedef struct qloco_a1_ctrl_params {
  double counter_per_gait, counter_per_swing; /* 240, 120 */
  double gait_counter_speed[4];               /* 2 */
  double gait_counter_reset[4];               /* gait_counter_reset(): 0, 120, 120, 0 */
  double default_foot_pos[12];
  double control_dt;                          /* 0.0025 */
  double kp_foot[12], kd_foot[12], km_foot[3], torques_gravity[12];
  double foot_delta_x_limit, foot_delta_y_limit; /* 0.1, 0.1 */
  double foot_force_low;                         /* FOOT_FORCE_LOW 30 */
  double foot_swing_clearance1, foot_swing_clearance2; /* (double)0.0f, (double)0.4f */
  int32_t recent_contact_window; /* 60, at most QLOCO_A1_CTRL_RC_WINDOW_MAX  */
  int32_t terrain_window;        /* 100, at most QLOCO_A1_CTRL_TER_WINDOW_MAX */
  int32_t torque_holdoff_ticks;  /* 10: torques are zero while mpc_init_counter < 10 */
  int32_t reserved[5];
} qloco_a1_ctrl_params;
void qloco_a1_ctrl_params_default(qloco_a1_ctrl_params *p);
/* The member state of every robot lives in a device workspace of
 * qloco_a1_ctrl_workspace_bytes(batch) bytes (-1 for batch <= 0), field-major
 * with slot-major filter rings.  get_state / set_state move it out of / into
 * a dense array of QLOCO_A1_CTRL_STATE doubles per robot (flags and counts as
 * 0.0 / 1.0 / integers in doubles):
 *   [0:4] gait_counter | [4:8] plan_contacts | [8:12] early_contacts |
 *   [12:16] contacts | [16:28] foot_pos_start | [28:40] foot_pos_rel_last_time |
 *   [40:52] foot_pos_target_last_time | [52:64] foot_pos_target_rel |
 *   [64:76] foot_pos_recent_contact | [76:88] foot_forces_kin |
 *   [88:100] joint_torques (the value the NaN guard holds) |
 *   [100] mpc_init_counter | [101] terrain_pitch_angle |
 *   recent-contact filters: [102:106] fill count per leg | [106:110] index of
 *   the oldest slot per leg | [110:122] sum_ | [122:134] correction_ (3x4) |
 *   terrain filter: [134] fill | [135] oldest slot | [136] sum_ | [137] correction_ |
 *   [138:858] recent-contact ring, 60 slots x 12 | [858:958] terrain ring.
 * The x, y and z filters of a leg always advance together and share fill
 * count and head.  The deque of MovingWindowFilter is slots head, head + 1,
 * ... (mod window), fill of them. */
#define QLOCO_A1_CTRL_STATE 958
#define QLOCO_A1_CTRL_RC_WINDOW_MAX 60
#define QLOCO_A1_CTRL_TER_WINDOW_MAX 100
int64_t qloco_a1_ctrl_workspace_bytes(int64_t batch);
/* The A1CtrlStates::reset() / constructor values: everything zero, the gait
 * counters at gait_counter_reset, empty filters. */
int qloco_a1_ctrl_reset(const qloco_a1_ctrl_params *prm, int64_t batch, void *workspace,
                        void *stream);
/* update_plan then generate_swing_legs_ctrl, one tick of every robot.  Device
 * pointers: dt[B], movement_mode[B] (int32; 0 standstill), root_pos[B*3],
 * root_lin_vel[B*3], root_lin_vel_d[B*3], root_rot_mat[B*9], root_rot_mat_z
 * [B*9] (3x3 col-major), foot_pos_abs[B*12] (3x4 col-major), foot_force[B*4].
 * Outputs: contacts[B*4] (uint8) required -- the `contacts` input of sections
 * 9 and 1; optional (NULL): plan_contacts / early_contacts [B*4] (uint8),
 * gait_counter[B*4], foot_pos_target_rel / _abs / _world [B*12],
 * foot_pos_cur[B*12], foot_forces_kin[B*12], foot_pos_recent_contact[B*12]. */
int qloco_a1_ctrl_plan_swing(const qloco_a1_ctrl_params *prm, int64_t batch, void *workspace,
                             const double *dt, const int32_t *movement_mode,
                             const double *root_pos, const double *root_lin_vel,
                             const double *root_lin_vel_d, const double *root_rot_mat,
                             const double *root_rot_mat_z, const double *foot_pos_abs,
                             const double *foot_force, uint8_t *contacts, uint8_t *plan_contacts,
                             uint8_t *early_contacts, double *gait_counter,
                             double *foot_pos_target_rel, double *foot_pos_target_abs,
                             double *foot_pos_target_world, double *foot_pos_cur,
                             double *foot_forces_kin, double *foot_pos_recent_contact,
                             void *stream);
/* Terrain pitch: fits the plane through the workspace's
 * foot_pos_recent_contact, filters its angle against the ground plane (only
 * while root_pos[2] > 0.1), clamps to +-0.5 and writes root_euler_d[B*3]
 * entry 1 (in/out; the other entries are not touched).  Outputs:
 * terrain_pitch_angle[B]; surf_coef[B*3] optional. */
int qloco_a1_ctrl_terrain(const qloco_a1_ctrl_params *prm, int64_t batch, void *workspace,
                          const double *root_pos, double *root_euler_d,
                          double *terrain_pitch_angle, double *surf_coef, void *stream);
/* compute_joint_torques: j_foot[B*36] as section 11 writes it,
 * foot_forces_grf[B*12] as sections 1 and 9 write it (body frame, 3x4
 * col-major); reads contacts and foot_forces_kin from the workspace.
 * Output: joint_torques[B*12]. */
int qloco_a1_ctrl_joint_torques(const qloco_a1_ctrl_params *prm, int64_t batch, void *workspace,
                                const double *j_foot, const double *foot_forces_grf,
                                double *joint_torques, void *stream);
/* Dense state[B * QLOCO_A1_CTRL_STATE] out of / into the workspace. */
int qloco_a1_ctrl_get_state(int64_t batch, const void *workspace, double *state, void *stream);
int qloco_a1_ctrl_set_state(int64_t batch, void *workspace, const double *state, void *stream);

/* ====================================================================== */
/* 14. slow planner's step-timing SQP, batched (fp64)                      */
/*    replaces NLPClass::step_timing_opti_loop (unitree_ros/mosek_nlp_kmp/ */
/*    src/NLP/NLPClass_sqp.cpp:693-1102) with the parts of FootStepInputs / */
/*    Initialize it reads (:51-77, :131-138, :160-206, :212-216, :243-306), */
/*    Indexfind (:1105-1141), step_timing_object_function (:1144-1173),     */
/*    step_timing_constraints (:1175-1458) and solve_stepping_timing        */
/*    (:1619-1638): three SQP passes over a QP with 4 variables, 1 equality */
/*    and 24 inequalities (EiQuadProg), then the _ts / _tx / foot-location  */
/*    / CoM boundary-state updates and three samples of the LIP CoM.  The   */
/*    producer of the ts / tx inputs of section 8.  Not computed:           */
/*    CoM_height_solve (:2361) and with it _comz, ZMP and DCM; the          */
/*    _nTdx > 3 tail of the CoM roll-out; Foot_trajectory_solve; KMP.       */
/*    Section 15 adds CoM_height_solve, ZMP / DCM and the swing feet.       */
/* ====================================================================== */
/* Defaults: NLPClass.h:32-37, the "go1" branch of Initialize (:243-306) and
 * the robot constants NLPRTControlClass.cpp:33-56 passes (FOOT_WIDTH = 0.03
 * there, not the 0.01 of robot_const_para_config.cpp). */
typedef struct qloco_nlp_params {
  double dt, tstep;                 /* 0.025, 0.7 */
  double t_min, t_max;              /* 0.5, 1 */
  double footx_vmax, footx_vmin, footy_vmax, footy_vmin; /* 3, -2.875, 2, -1 */
  double comax_max, comax_min, comay_max, comay_min;     /* 5, -5, 6, -6 */
  double aax, aay, aaxv, aayv, bbx, bby, rr1, rr2;       /* objective weights */
  double footx_max, footx_min;      /* 0.15, -0.05 */
  double z_c, g, half_hip_width, foot_width; /* 0.309458, 9.8, 0.12675, 0.03 */
  double lamda_comx, lamda_comvx, lamda_comy, lamda_comvy; /* feedback blend (:980-983), 0 */
  double reserved[2];
} qloco_nlp_params;
void qloco_nlp_params_default(qloco_nlp_params *p);
/* Every robot's members live in a device workspace of
 * qloco_nlp_workspace_bytes(batch) bytes (-1 for batch <= 0).  Its first
 * 2 * B * 27 doubles are ts[B*27] then tx[B*27], a row per robot: the arrays
 * qloco_support_phase takes, so the two calls chain with no copy.  The rest is
 * field-major.  get_state / set_state move a dense record of QLOCO_NLP_STATE
 * doubles per robot:
 *   [0:27] _ts | [27:54] _tx | [54:81] _td | [81:108] _Lxx_ref |
 *   [108:135] _Lyy_ref | [135:162] _footx_ref | [162:189] _footy_ref |
 *   [189:216] _COMx_is | [216:243] _COMvx_is | [243:270] _COMy_is |
 *   [270:297] _COMvy_is | [297:301] _Vari_ini.col(i-1) |
 *   [301:307] _comx/_comvx/_comax/_comy/_comvy/_comay _feed(i-1) |
 *   [307:309] _comvx_endref, _comvy_endref */
#define QLOCO_NLP_STATE 309
/* per-pass code beside the qloco_status values of the solver, and the
 * per-robot status of a robot whose _periond_i would pass 26 */
#define QLOCO_NLP_SKIPPED (-1)
#define QLOCO_NLP_FINISHED (-2)
int64_t qloco_nlp_workspace_bytes(int64_t batch);
/* FootStepInputs + Initialize for B robots: steplength[B], stepwidth[B]
 * (device; the reference passes 0.075 and 2 * half_hip_width); stepheight[B]
 * is optional (it only reaches _footz_ref, which the SQP never reads). */
int qloco_nlp_init(const qloco_nlp_params *prm, int64_t batch, void *workspace,
                   const double *steplength, const double *stepwidth, const double *stepheight,
                   void *stream);
/* One planner tick of every robot.  Device pointers: t_int[B] (int32, the
 * loop index i >= 1), estimated_state[B*6] (elements 0..5), rfoot_feedback /
 * lfoot_feedback[B*2] (x, y).  Outputs: vari_ini[B*4] required; optional
 * (NULL): sched[B*4] (int32: _periond_i, _k_yu, _bjxx, _bjx1), step[B*3]
 * (_ts(_periond_i-1), _Lxx_ref(_periond_i-1), _Lyy_ref(_periond_i-1) after the
 * update), com[B*18] (for i, i+1, i+2: comx, comy, comvx, comvy, comax,
 * comay), pass_status / pass_iters[B*3] (per SQP pass: the EiQuadProg outcome
 * -- QLOCO_INFEASIBLE's partial iterate is added, as the reference does -- or
 * QLOCO_NLP_SKIPPED, and the iteration count), status[B]: QLOCO_OK, QLOCO_NAN
 * (a non-finite result, carried into the record), QLOCO_NLP_FINISHED or
 * QLOCO_BAD_SIZE (i < 1 or before the plan); the last two leave the record
 * untouched and return NaN. */
int qloco_nlp_step_timing(const qloco_nlp_params *prm, int64_t batch, void *workspace,
                          const int32_t *t_int, const double *estimated_state,
                          const double *rfoot_feedback, const double *lfoot_feedback,
                          double *vari_ini, int32_t *sched, double *step, double *com,
                          int32_t *pass_status, int32_t *pass_iters, int32_t *status,
                          void *stream);
/* Dense state[B * QLOCO_NLP_STATE] out of / into the workspace. */
int qloco_nlp_get_state(int64_t batch, const void *workspace, double *state, void *stream);
int qloco_nlp_set_state(int64_t batch, void *workspace, const double *state, void *stream);
/* Lanes per robot of the tick kernel: 4 (default), 8 or 16; results do not
 * depend on it.  Returns the previous width, or QLOCO_ERR_ARG. */
int qloco_nlp_set_group_width(int gw);

/* ====================================================================== */
/* 15. the rest of the slow planner's tick, batched (fp64)                 */
/*    completes section 14 up to the NLPClass boundary: CoM_height_solve   */
/*    (NLPClass_sqp.cpp:2361-2473, called at :936 with the _bjx1 of the     */
/*    previous tick) and with it _comz / _comvz / _comaz, the ZMP and DCM   */
/*    samples (:950-954, _Zsc of :323-328), all 38 slots of com_traj        */
/*    (:1048-1090) and Foot_trajectory_solve_mod2 (:2039-2358) with         */
/*    solve_AAA_inv2 (:3633-3644).  One call launches section 14's kernel   */
/*    unchanged and then one kernel of its own on the same stream.  Not     */
/*    computed: Zmp_distributor / Force_torque_calculate, the               */
/*    _state_generate_interpo packing, KMP and foot rotation, the unused    */
/*    Foot_trajectory_solve, the _nTdx > 3 tail.                            */
/* ====================================================================== */
/* Defaults: _lift_height = 0.03 (NLPRTControlClass.cpp:48); _hcom =
 * RobotPara_Z_C - _height_offset = 0.309458 (NLPClass_sqp.cpp:212,
 * NLPClass.h:37, robot_const_para_config.cpp:14). */
typedef struct qloco_nlp_tick_params {
  double lift_height, hcom;
  double reserved[6];
} qloco_nlp_tick_params;
void qloco_nlp_tick_params_default(qloco_nlp_tick_params *p);
/* The members section 14's record lacks live in a second device workspace of
 * qloco_nlp_tick_workspace_bytes(batch) bytes (-1 for batch <= 0), field-major
 * (field f of robot b at f * B + b), followed by scratch for the step-timing
 * outputs the caller does not ask for.  get_state / set_state move a dense
 * record of QLOCO_NLP_TICK_STATE doubles per robot (integers as doubles):
 *   [0] _bjx1 of the previous tick | [1] _ry_left_right | [2] _t_end_footstep |
 *   [3] _stepwidth(0) | [4] the loop index of the last tick |
 *   [5:32] _footz_ref | [32:59] _lift_height_ref | [59:86] the initial _tx
 *   (for _Zsc) | [86:374] a ring of QLOCO_NLP_TICK_RING entries of
 *   (_Rfootx, _Rfooty, _Rfootz, _Lfootx, _Lfooty, _Lfootz): array index k is
 *   entry k % QLOCO_NLP_TICK_RING.
 * The ring replaces the reference's arrays of _nsum entries: a tick reads no
 * further back than round(_tx(_bjx1-1)/_dt) - 2, so the ring has to hold
 * round(t_max / dt) ticks, that look-back and the forecast slot; init and tick
 * return QLOCO_ERR_ARG when round(t_max / dt) + 4 exceeds it.  An index past
 * the last tick + 1 reads as Initialize left the arrays (:496-499), one the
 * ring no longer holds as NaN (reported as QLOCO_NAN).  The loop index is
 * expected to advance by one per call, as in the reference. */
#define QLOCO_NLP_TICK_RING 48
#define QLOCO_NLP_TICK_STATE 374
int64_t qloco_nlp_tick_workspace_bytes(int64_t batch);
/* qloco_nlp_init on nlp_workspace, then the second workspace.  stepheight[B]
 * NULL: flat ground. */
int qloco_nlp_tick_init(const qloco_nlp_params *prm, const qloco_nlp_tick_params *tick_prm, int64_t batch,
                        void *nlp_workspace, void *tick_workspace, const double *steplength,
                        const double *stepwidth, const double *stepheight, void *stream);
/* One planner tick of every robot: step_timing_opti_loop followed by
 * Foot_trajectory_solve_mod2 with the same loop index (NLPRTControlClass.cpp:
 * 445-459).  Inputs as qloco_nlp_step_timing, plus stop_walking[B] (int32,
 * NULL = 0).  Outputs: com_traj[B*38], every slot as :1048-1090 fills it
 * (28..33 NaN on the plan's last step, where the reference reads past the
 * end); rlfoot_traj[B*18] (R xyz, L xyz, R v, L v, R a, L a; velocity and
 * acceleration entries the reference does not write on a tick are 0);
 * right_support[B] (0 left support, 1 right support, 2 double support);
 * vari_ini[B*4] and the optional sched / step / com / pass_status /
 * pass_iters of section 14, written by its kernel; status[B] (optional):
 * section 14's status, or QLOCO_NAN when a value of this section is not
 * finite.  A robot whose step-timing status is QLOCO_NLP_FINISHED or
 * QLOCO_BAD_SIZE leaves both records untouched and returns NaN with
 * right_support 2. */
int qloco_nlp_tick(const qloco_nlp_params *prm, const qloco_nlp_tick_params *tick_prm, int64_t batch,
                   void *nlp_workspace, void *tick_workspace, const int32_t *t_int,
                   const double *estimated_state, const double *rfoot_feedback,
                   const double *lfoot_feedback, const int32_t *stop_walking, double *com_traj,
                   double *rlfoot_traj, int32_t *right_support, double *vari_ini, int32_t *sched,
                   double *step, double *com, int32_t *pass_status, int32_t *pass_iters, int32_t *status,
                   void *stream);
/* Form of the new kernel: 1 = one robot per lane (default), 8 = one robot per
 * 8-lane group with a row of the 7 x 7 system per lane; results do not depend
 * on it.  Returns the previous value, or QLOCO_ERR_ARG. */
int qloco_nlp_tick_set_group_width(int gw);
/* Dense state[B * QLOCO_NLP_TICK_STATE] out of / into the second workspace. */
int qloco_nlp_tick_get_state(int64_t batch, const void *tick_workspace, double *state, void *stream);
int qloco_nlp_tick_set_state(int64_t batch, void *tick_workspace, const double *state, void *stream);

/* ====================================================================== */
/* 16. go1 servo tick, batched (fp64): joint state, IMU quaternion and the */
/*    /MPC/Gait row in, joint commands, torques and /control2rtmpc/state   */
/*    out.  Replaces one iteration of the sim servo loop, go1_rt_control/  */
/*    src/servo_control/servo.cpp:675-1330, and the go1_gait_data row of   */
/*    :1333-1433: quat_to_euler + Forward_kinematics_g x 4 (:690-741), the */
/*    measured foot velocity (:749-755), the state row (:758-762), the     */
/*    stand-up branch (:769-809) or the gait branch (:889-1051: counters,  */
/*    15 Butterworth filters, per-mode targets, Inverse_kinematics_g x 4)  */
/*    followed by section 7's force block (:1052-1243), the joint commands */
/*    (:1265-1296) and the end-of-loop updates (:1318-1330).  Not          */
/*    computed: root_rot_mat / root_rot_mat_z (never read), the callbacks  */
/*    and publishers, the hardware loop (torque_mode.cpp).                 */
/* ====================================================================== */
/* One second-order Butterworth low-pass (Filter/butterworthLPF.cpp:83-120):
 * init()'s coefficients, computed on the host with its expressions and its
 * 3.14159265359; the kernel never calls tan. */
typedef struct qloco_butter_coef {
  double b0, b1, b2, a1, a2, a;
} qloco_butter_coef;
/* The 15 live filters in the loop's order (index: reference filter, gait slot):
 *   0-2  LPF1-3   com_des       slots 0-2      3 Hz
 *   3-5  LPF7-9   rfoot_des     slots 9-11     3 Hz
 *   6-8  LPF10-12 lfoot_des     slots 6-8      3, 3, 10 Hz (:593, kept)
 *   9-11 LPF13-15 coma_des      slots 39-41    10 Hz
 *  12-14 LPF16-18 thetaacc_des  slots 73-75    10 Hz */
#define QLOCO_GO1_SERVO_FILTERS 15
typedef struct qloco_go1_servo_params {
  double rt_frequency;    /* 1000     servo.cpp:633 (time_programming = 1 / it) */
  double stand_duration;  /* 5        :639 */
  double dtx;             /* 0.005    gait::t_program_cyclic (:567) */
  double dt_mpc_slow;     /* 0.025    n_t_int = round(dt_mpc_slow / dtx) (:568) */
  double t_period;        /* 0.7      n_period = round(t_period / dtx) (:616) */
  double t_walk_start;    /* 0.6      the gate of :933 */
  double pi;              /* 3.141526 gait::pi (sic), mode 103's pitch (:998) */
  double half_hip_width;  /* 0.12675  RobotParaClass_HALF_HIP_WIDTH */
  double z_c;             /* 0.309458 gait::Z_c: com_des(2) of paramInit (:450) */
  double target_pos[12];  /* :767 */
  qloco_butter_coef filter[QLOCO_GO1_SERVO_FILTERS];
  qloco_force_params force;  /* the Dynamiccclass constants of section 3 */
  double reserved[8];        /* room for the hardware loop's constants */
} qloco_go1_servo_params;
void qloco_go1_servo_params_default(qloco_go1_servo_params *p);

/* Per-robot state, as get_state / set_state move it: a dense record of
 * QLOCO_GO1_SERVO_STATE doubles (integers and flags as doubles):
 *   [0:75]    the 15 filters, 5 each: y_p, y_pp, x_p, x_pp, i (calls, <= 3)
 *   [75:87]   angle_des (FR, FL, RR, RL)   [87:99]   FR..RL_foot_Homing
 *   [99:102]  body_p_Homing                [102:105] body_p_des
 *   [105:108] body_r_des                   [108:120] FR..RL_foot_des
 *   [120:132] foot_relative_des_old        [132:144] foot_relative_mea_old
 *   [144:147] com_des_pre                  [147:159] v_relative
 *   [159:171] v_est_relative               [171]     count_in_rt_loop
 *   [172:176] FR..RL_swing                 [176:188] F_leg_ref (3 x 4 col-major)
 *   [188:200] grf_opt                      [200:212] Legs_torque
 *   [212:230] com_des, rfoot_des, lfoot_des, coma_des, thetaacc_des, comv_des
 *   [230]     state_feedback(0) = t_int    [231:237] Force_L_R
 *   [237:243] F_sum                        [243:279] FR..RL_Jaco (col-major)
 *   [279]     qp_solution  [280] EiQuadProg status  [281:288] 0
 * The force QP's grouping workspace is a cache, not state: results are
 * bit-identical with or without it, and set_state leaves it alone. */
#define QLOCO_GO1_SERVO_STATE 288
#define QLOCO_GO1_GAIT_DATA_LEN 100
/* Optional device outputs of a tick (any may be NULL), [B * n] each: the
 * reference's members of the same names after the tick. */
typedef struct qloco_go1_servo_diag {
  double *body_r_est;   /* 3 */
  double *foot_rel_mea; /* 12 */
  double *v_est_rel;    /* 12 */
  double *Jaco_est;     /* 36 */
  double *com_des, *rfoot_des, *lfoot_des, *coma_des, *thetaacc_des, *comv_des; /* 3 each */
  double *body_p_des, *body_r_des; /* 3 each */
  double *foot_des;     /* 12 */
  double *angle_des;    /* 12 */
  double *Jaco;         /* 36 */
  int32_t *ik_updates;  /* 4: Newton steps applied per leg (0 while standing up) */
  double *F_sum, *Force_L_R; /* 6 each */
  int32_t *swing;       /* 4 */
  int32_t *qp_solution, *status; /* 1 each */
} qloco_go1_servo_diag;
/* Bytes of the device workspace of B robots (-1 for batch <= 0). */
int64_t qloco_go1_servo_workspace_bytes(int64_t batch);
/* paramInit (:300-470) and the member setup of main (:556-616) for B robots. */
int qloco_go1_servo_init(const qloco_go1_servo_params *prm, int64_t batch, void *workspace,
                         void *stream);
/* One loop iteration of B robots started together.  n_count: the node's loop
 * counter (host; the caller increments it), so the branch of :769 is uniform
 * over the batch and count_in_rt_ros = n_count + 1; count_in_rt_loop is
 * per-robot state.  Device inputs: q_mea[B*12] (lowState.motorState[j].q),
 * quat[B*4] (w, x, y, z), gait_msg[B*100] (the latest /MPC/Gait row),
 * gait_mode[B] (int32), y_offset[B].  Device outputs: q_cmd[B*12],
 * ctrl_msg[B*25] (the row published at :762, i.e. [0] = the previous tick's
 * t_int, the rest 0), tau[B*12] (Legs_torque), grf_opt[B*12]; optional
 * diag and gait_data[B*100] ([0:90] as :1335-1433 writes them, the rest 0).
 * While standing up the force QP is not launched: tau, grf_opt and the swing
 * flags keep their values. */
int qloco_go1_servo_tick(const qloco_go1_servo_params *prm, int64_t batch, void *workspace,
                         int64_t n_count, const double *q_mea, const double *quat,
                         const double *gait_msg, const int32_t *gait_mode, const double *y_offset,
                         double *q_cmd, double *ctrl_msg, double *tau, double *grf_opt,
                         const qloco_go1_servo_diag *diag, double *gait_data, void *stream);
/* The tick with per-robot bodies (section 3's qloco_force_body; device, `batch`
 * rows, or NULL = qloco_go1_servo_tick, which forwards here).  Only the gait
 * branch reads the rows, with the meaning and the refused-row rule of
 * qloco_servo_force_block_body (the caller's tau and grf_opt rows of a refused
 * robot are NaN; the workspace stays finite).  While the batch stands up no QP
 * is launched, the rows are not read and nothing is refused. */
int qloco_go1_servo_tick_body(const qloco_go1_servo_params *prm, int64_t batch, void *workspace,
                              int64_t n_count, const double *q_mea, const double *quat,
                              const double *gait_msg, const int32_t *gait_mode,
                              const double *y_offset, double *q_cmd, double *ctrl_msg, double *tau,
                              double *grf_opt, const qloco_go1_servo_diag *diag, double *gait_data,
                              const qloco_force_body *body, void *stream);
/* Dense state[B * QLOCO_GO1_SERVO_STATE] out of / into the workspace. */
int qloco_go1_servo_get_state(int64_t batch, const void *workspace, double *state, void *stream);
int qloco_go1_servo_set_state(int64_t batch, void *workspace, const double *state, void *stream);

/* ====================================================================== */
/* 17. slow planner node tick, batched (fp64): /rt2nrt/state in, the       */
/*    /MPC/Gait row out.  Replaces one iteration of the node loop,         */
/*    unitree_ros/mosek_nlp_kmp/src/gait_nlp_kmp.cpp:40-60, 101-158, and   */
/*    NLPRTControlClass::WalkingReactStepping / rt_nlp_gait                */
/*    (NLPRTControl/NLPRTControlClass.cpp:191-396, :436-596) around        */
/*    section 15's tick, which is launched unchanged: the start latch and  */
/*    loop counter, the branch (not started, squat, walking, over time,    */
/*    stopped), X_CoM_position_squat (NLPClass_sqp.cpp:2958-3015),         */
/*    Zmp_distributor / zmp_interpolation / Force_torque_calculate         */
/*    (:3650-3895) with the _nTdx > 3 tail of the ZMP roll-out (:938-951)  */
/*    they read, and the 100-slot row (:288-392).  Not computed: KMP, foot */
/*    rotation, XGetSolution_*, StartWalking / StopWalking (the node never */
/*    calls them).                                                         */
/* ====================================================================== */
/* Defaults: NLPRTControlClass.h:16-18, NLPClass.h:37-38,
 * NLPRTControlClass.cpp:34 and the "go1" _rad of Initialize (:275). */
typedef struct qloco_nlp_node_params {
  double dtx;                 /* 0.025  _dtx = dt_nlp; has to equal qloco_nlp_params.dt */
  double height_offset_time;  /* 1 */
  double height_squat_time;   /* 1 */
  double height_offset;       /* 0      _height_offset of the squat polynomial */
  double height_offsetx;      /* 0      _height_offsetx (only reaches _COM_IN, which nothing reads) */
  double totalmass;           /* 12     RobotPara_totalmass = _mass */
  double rad;                 /* 0.2    _j_ini = _mass * _rad^2 */
  double reserved[9];
} qloco_nlp_node_params;
void qloco_nlp_node_params_default(qloco_nlp_node_params *p);
/* The node's members live in a third device workspace of
 * qloco_nlp_node_workspace_bytes(batch) bytes (-1 for batch <= 0): the record,
 * field-major (field f of robot b at f * B + b), then the scratch the inner
 * tick writes.  get_state / set_state move a dense record of
 * QLOCO_NLP_NODE_STATE doubles per robot (integers and flags as doubles):
 *   [0] count | [1] mpc_start (latched) | [2] _t_walkdtime_restart_flag |
 *   [3] mpc_stop | [4:7] diagonal of _Co_L | [7:10] diagonal of _Co_R |
 *   [10:154] a ring of QLOCO_NLP_NODE_RING entries of (tag, _zmpx_real,
 *   _zmpy_real): array index k lives in entry k % QLOCO_NLP_NODE_RING and the
 *   tag is the array index the entry holds (-1: none) |
 *   [154:254] the last row: every member WalkingReactStepping packs
 *   (PelvisPos, the feet, zmp_ref, F_L, F_R, M_L, M_R, bjx1, dcm_ref,
 *   PelvisPosv / a, mpc_body(13..37), mpc_rlfoot_traj(6..17), mpc_stop,
 *   right_support) lives in its slot of the row and nowhere else.
 * The ring replaces the reference's _zmpx_real / _zmpy_real of _nsum entries,
 * kept "as last written": a tick writes entries i .. i + _nTdx - 1 and reads
 * i, i - 1, round(_tx(_bjx1-1)/_dt) - 2 and round((_tx+_td)(_bjx1-1)/_dt) - 1,
 * the last two only in the double-support ticks of a step, so the span fits
 * as section 15's does.  An index no tick has written reads 0 (Initialize,
 * :526); one whose entry a later index has taken reads NaN (QLOCO_NAN).
 * Scratch, in doubles from the end of the records (offset * B, [B * n] each,
 * row-major): 0 com_traj (38) | 38 rlfoot_traj (18) | 56 com (18) |
 * 74 vari_ini (4) | 78 the zero estimated_state (6) | 84 rfoot_feedback (2) |
 * 86 lfoot_feedback (2) | 88 the _bjx1 and _td(1) of before the tick (2) |
 * 90, as int32: t_int[B], right_support[B], section 14's sched[B*4],
 * the tick's status[B], branch[B]. */
#define QLOCO_NLP_NODE_RING 48
#define QLOCO_NLP_NODE_STATE 254
#define QLOCO_NLP_NODE_SCRATCH 94
/* sched[B*8] (int32, optional): the branch, _walkdtime1, _t_int (0: section 15
 * did not tick), bjx1, status, count, _nTdx (0 unless walking), the array
 * index of ZMP_end (-1 unless Zmp_distributor interpolates). */
#define QLOCO_NLP_NODE_SCHED_LEN 8
#define QLOCO_NLP_NODE_NOT_STARTED 0
#define QLOCO_NLP_NODE_SQUAT 1
#define QLOCO_NLP_NODE_WALKING 2
#define QLOCO_NLP_NODE_OVER_TIME 3
#define QLOCO_NLP_NODE_STOPPED 4
int64_t qloco_nlp_node_workspace_bytes(int64_t batch);
/* qloco_nlp_tick_init on the first two workspaces, then NLPRTControlClass()
 * (:86-185) on the third. */
int qloco_nlp_node_init(const qloco_nlp_params *prm, const qloco_nlp_tick_params *tick_prm,
                        const qloco_nlp_node_params *node_prm, int64_t batch, void *nlp_workspace,
                        void *tick_workspace, void *node_workspace, const double *steplength,
                        const double *stepwidth, const double *stepheight, void *stream);
/* One iteration of the node loop of every robot, three launches on one stream
 * and no host step: a kernel that reads nrt_msg[B*25] (the latest /rt2nrt/state
 * row: [0] > 0 starts the robot and advances its count, [19..21] / [22..24] the
 * left / right foot feedback), picks the branch and writes the t_int section 15
 * takes (0 for a robot that does not walk this tick, which section 15 answers
 * with QLOCO_BAD_SIZE and untouched records); qloco_nlp_tick, with zeros for
 * estimated_state as rt_nlp_gait passes them; a kernel that writes
 * gait_msg[B*100], the /MPC/Gait row ([98] = 0, the node's wall-clock duration).
 * A stopped robot (mpc_stop >= 1) re-emits its last row.  status[B] (optional):
 * QLOCO_OK, section 15's status of a walking robot, or QLOCO_NAN when a slot
 * this section computes is not finite. */
int qloco_nlp_node_tick(const qloco_nlp_params *prm, const qloco_nlp_tick_params *tick_prm,
                        const qloco_nlp_node_params *node_prm, int64_t batch, void *nlp_workspace,
                        void *tick_workspace, void *node_workspace, const double *nrt_msg,
                        double *gait_msg, int32_t *sched, int32_t *status, void *stream);
/* Form of the row store: 0 = each lane writes its robot's row, 1 = the wave
 * stages 16 rows at a time through LDS and writes them coalesced (default);
 * results do not depend on it.  Returns the previous value, or QLOCO_ERR_ARG. */
int qloco_nlp_node_set_form(int form);
/* Dense state[B * QLOCO_NLP_NODE_STATE] out of / into the third workspace. */
int qloco_nlp_node_get_state(int64_t batch, const void *node_workspace, double *state, void *stream);
int qloco_nlp_node_set_state(int64_t batch, void *node_workspace, const double *state, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* QLOCO_H */

/*
 * include/qrw_hip.h — C ABI of libqrw_hip.so, the MI355X (gfx950) implementation of the
 * quadruped-reactive-walking control-loop hot path, batched over B independent Solo12
 * instances.  Plain pointers and sizes only; no C++ or torch types cross this boundary.
 *
 * Each entry point names the reference interface it replaces (paths under
 * /root/reference).  In the reference these are Boost.Python/eigenpy bound C++ methods
 * (python/gepadd.cpp) called from scripts/MPC_Wrapper.py and scripts/QP_WBC.py; here the
 * same calls arrive through ctypes (see INTEGRATION.md for the binding a maintainer adds).
 *
 * Conventions
 *   - all arrays are C-order (row-major) doubles with the reference's own shapes and a
 *     leading batch dimension B; `d_` pointers are device (HBM) pointers, `h_` host pointers;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); device-pointer
 *     entry points only enqueue work and never synchronise or allocate;
 *   - every function returns 0 on success, <0 on error (qrw_last_error() has the text);
 *     like the reference (src/MPC.cpp:558,648; src/QPWBC.cpp:270,389) a solver that stops
 *     at max-iter or detects infeasibility is NOT an error: its status is reported per
 *     instance through qrw_*_get_stats and the (possibly NaN) result is passed through;
 *   - a handle owns the per-instance persistent solver state (warm start, rho, stale
 *     B/S entries — SURVEY.md §0.4) of ONE GPU's shard; single caller, not thread-safe;
 *   - synchronisation is per handle, never device-wide: a `_host` entry point or a getter waits for the last launch of the
 *     state it reads (on whatever stream the caller launched it) and for its own copies on a private non-blocking stream of
 *     the handle -- another handle's (or anybody's) work in flight on other streams is neither waited for nor stalled;
 *   - entry points that exist for the test suite only are declared in include/qrw_hip_test.h.
 */
#ifndef QRW_HIP_H_
#define QRW_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qrw_handle_s *qrw_handle;

typedef struct {
  int32_t batch;   /* B: instances owned by this handle                                  */
  int32_t n_steps; /* N: MPC horizon steps, MPC::MPC n_steps_in (src/MPC.cpp:3); 1..32   */
  int32_t N_gait;  /* rows of fsteps / gait matrices, MPC::MPC N_gait; >= n_steps        */
  int32_t device;  /* HIP device ordinal                                                  */
  double dt_mpc;   /* MPC::MPC dt_in (src/config_solo12.yaml:11 -> 0.02)                  */
  double T_gait;   /* MPC::MPC T_gait_in (unused by the maths, kept for the call surface) */
  double dt_wbc;   /* wbc_controller dt / InvKin dt (scripts/QP_WBC.py:18 -> 0.002)       */
} qrw_config;

/* solver status values (OSQP constants, as ignored by src/MPC.cpp:558) */
#define QRW_STATUS_SOLVED 1
#define QRW_STATUS_SOLVED_INACCURATE 2
#define QRW_STATUS_MAX_ITER_REACHED (-2)
#define QRW_STATUS_PRIMAL_INFEASIBLE (-3)
#define QRW_STATUS_DUAL_INFEASIBLE (-4)
#define QRW_STATUS_NON_CVX (-7)
#define QRW_STATUS_UNSOLVED (-10)
#define QRW_STATUS_NOT_SETUP (-100) /* run with num_iter != 0 before any num_iter == 0 call */

/* Replaces the constructors MPC::MPC (src/MPC.cpp:3-32; binding python/gepadd.cpp:22-24),
 * QPWBC::QPWBC (src/QPWBC.cpp:4-30; python/gepadd.cpp:217) and InvKin::InvKin
 * (src/InvKin.cpp:3-10; python/gepadd.cpp:186) for a batch of B instances. */
int qrw_create(const qrw_config *cfg, qrw_handle *out);
int qrw_destroy(qrw_handle h);
const char *qrw_last_error(void);

/* Replaces MPC::run(num_iter, xref_in, fsteps_in) + MPC::get_latest_result()
 * (src/MPC.cpp:626-649,604; python/gepadd.cpp:27-29), i.e. what
 * MPC_Wrapper.run_MPC_synchronous does (scripts/MPC_Wrapper.py:142,148), per instance.
 *   d_xref     [B][12][N+1]   column 0 = current state
 *   d_fsteps   [B][N_gait][12] row i = horizon step i, zero = swing / beyond horizon
 *   d_num_iter [B] int32 or NULL; if NULL num_iter_scalar applies to every instance.
 *              num_iter == 0 (re)creates the QP and cold-starts the solver (MPC.cpp:636-637)
 *   d_out      [B][24][N]     x_f_applied: rows 0-11 predicted states, 12-23 forces
 * Scheduling inside the call (no reference counterpart; never visible in the results): instances are started longest first by
 * a moving average of their previous iteration counts; at N > 16 with more instances than the device holds at a time, a
 * workgroup runs at most 600 ADMM iterations of a solve, then parks it (bit-exact resume) for one of the launch's taker
 * workgroups if one is still to come -- it goes on itself otherwise -- and the parked solves are taken
 * longest-predicted-remainder first, the prediction read off the decay of the residuals.  No workgroup waits for work that a
 * workgroup not yet running would have to produce (since round 5; a taker that finds nothing parked leaves).  d_out is
 * pre-filled with NaN then: should a parked solve not reach its taker (a queue overrun, or the few instructions between a
 * parker's reservation and its store taking 2 s -- never expected), the unfinished instances keep NaN, the kernel
 * leaves a code in a host-mapped word, and THE NEXT qrw_mpc_solve of the handle returns -12 once, without launching (no device
 * sync involved; qrw_mpc_get_stats reports it as well).  The call after that runs normally and starts the unfinished instances
 * cold (zero x, z, y, rho 0.1: what OSQP's store_solution leaves after a failed solve).  NaN forces stop the robot through the
 * controller's fourth error code (qrw_controller_result).  Environment knobs: INTEGRATION.md. */
int qrw_mpc_solve(qrw_handle h, const double *d_xref, const double *d_fsteps, const int32_t *d_num_iter,
                  int32_t num_iter_scalar, double *d_out, void *stream);
/* same with host buffers (H2D, solve, D2H, synchronised) — used by the single-robot drop-in */
int qrw_mpc_solve_host(qrw_handle h, const double *h_xref, const double *h_fsteps, const int32_t *h_num_iter,
                       int32_t num_iter_scalar, double *h_out);

/* MPC::get_gait / MPC::get_Sgait (src/MPC.cpp:770-780; python/gepadd.cpp:30-31) of instance b:
 * h_gait [N_gait][4], h_Sgait [12 N] */
int qrw_mpc_get_gait(qrw_handle h, int32_t b, double *h_gait, double *h_Sgait);

/* K consecutive MPC::run calls of every instance (call indices first_num_iter .. first_num_iter + K - 1) in ONE launch:
 * d_xref [K][B][12][N+1], d_fsteps [K][B][N_gait][12] -> d_out [K][B][24][N], d_iters [K][B] int32 (may be NULL).  Results
 * and the persistent solver state afterwards are those of K calls of qrw_mpc_solve, bit for bit; what differs is the
 * ordering: there is no device-wide barrier between the calls, only each instance's own order (a task queue hands call s+1
 * of an instance out when its call s has finished), so one instance's long solve delays nobody else's next call.  For
 * inputs that are all known beforehand — replaying the planner outputs a log holds (`planner_xref`, `planner_fsteps`,
 * scripts/LoggerControl.py:61-65,142-143) to recompute `mpc_x_f` (:76,:152), or open-loop evaluation sweeps — not for a
 * closed control loop, whose next inputs depend on this call's result.  A diagnostic for an out-of-scope consumer (log
 * replay), not part of the control path.  d_out is pre-filled with NaN and d_iters with -1, so a call that never ran cannot
 * be mistaken for a result.  qrw_mpc_sequence_error waits for the handle's sequence launch and reports whether any workgroup gave up
 * waiting for a task (2 s without ANY task of the sequence finishing -- the clock restarts on observed progress, so the
 * length of K or of one instance's chain does not matter; never expected).  Forward progress assumes that workgroups of one
 * launch start in index order (true of the hardware dispatcher; also on CU-masked streams, where fewer are resident). */
int qrw_mpc_solve_sequence(qrw_handle h, int32_t K, const double *d_xref, const double *d_fsteps, int32_t first_num_iter,
                           double *d_out, int32_t *d_iters, void *stream);
int qrw_mpc_sequence_error(qrw_handle h, int32_t *timed_out);

/* Device-to-device copy of the last solve's ADMM iteration counts (int32 [B]) on `stream`: lets a caller keep per-launch
 * work statistics in HBM without a host round trip inside a timed region (bench.py's roofline accounting).  No reference
 * counterpart: OSQP's info->iter is never read by the reference (src/MPC.cpp:558). */
int qrw_mpc_copy_iters(qrw_handle h, int32_t *d_iters, void *stream);

/* Per-instance solver statistics of the last qrw_mpc_solve (host arrays of B, any may be NULL).
 * The reference never inspects them (OSQP status ignored); exposed so the silent
 * pass-through can be observed (SURVEY.md §8(b) error convention). */
int qrw_mpc_get_stats(qrw_handle h, int32_t *h_iters, int32_t *h_status, double *h_rho, double *h_pri_res,
                      double *h_dua_res);

/* Diagnostic: OSQP-ordered copies of instance b's persisted scaled iterates x[24N], z[44N],
 * y[44N] and of the last solve's scaling D[24N], E[44N], c (any may be NULL). Tests only. */
int qrw_mpc_get_state(qrw_handle h, int32_t b, double *h_x, double *h_z, double *h_y, double *h_D, double *h_E,
                      double *h_c);

/* Diagnostic: the block order the NEXT qrw_mpc_solve will use (h_order[i] = instance solved by workgroup i: a
 * permutation of 0..B-1, longest predicted solve first) and the moving average of iteration counts it was sorted by
 * (either may be NULL).  *has_order = 0 while no order exists (batch <= 1024, or before the first solve).  Synchronises
 * the device.  No reference counterpart (scheduling only; results do not depend on it).  Tests only. */
int qrw_mpc_get_order(qrw_handle h, int32_t *h_order, float *h_ema, int32_t *has_order);

/* Diagnostic: bookkeeping of the last time-sliced qrw_mpc_solve (N > 16 with more instances than resident slots; all zero
 * otherwise): priority levels and slice length in use, solves parked into each level (level 0 = first parks), taker
 * workgroups that took a parked solve, instances counted as finished.  No reference counterpart. */
int qrw_mpc_get_slice_stats(qrw_handle h, int32_t *levels, int32_t *chunk, uint32_t *h_parks_per_level /* [9] */,
                            uint32_t *h_takers, uint32_t *h_finished);

/* Replaces wbc_controller.compute (scripts/QP_WBC.py:52-131) with everything it calls:
 * Solo12InvKin.refreshAndCompute (scripts/solo12InvKin.py:44-69), InvKin::refreshAndCompute
 * (src/InvKin.cpp:23-73), the Pinocchio crba/Jacobian/rnea calls (QP_WBC.py:89-116) and
 * QPWBC::run + getters (src/QPWBC.cpp:310-390,302-308; python/gepadd.cpp:219-223).
 *   in : d_q [B][19], d_dq [B][18], d_f_cmd [B][12], d_contacts [B][4],
 *        d_pgoals / d_vgoals / d_agoals [B][3][4]
 *   out: d_tau_ff [B][12], d_qdes [B][19], d_vdes [B][18], d_f_with_delta [B][12],
 *        d_ddq_res [B][6] (QPWBC::get_ddq_res), d_feet [B][3][3][4] = feet_pos, feet_err,
 *        feet_vel (QP_WBC.py:73-80); any output may be NULL */
int qrw_wbc_compute(qrw_handle h, const double *d_q, const double *d_dq, const double *d_f_cmd,
                    const double *d_contacts, const double *d_pgoals, const double *d_vgoals, const double *d_agoals,
                    double *d_tau_ff, double *d_qdes, double *d_vdes, double *d_f_with_delta, double *d_ddq_res,
                    double *d_feet, void *stream);
int qrw_wbc_compute_host(qrw_handle h, const double *h_q, const double *h_dq, const double *h_f_cmd,
                         const double *h_contacts, const double *h_pgoals, const double *h_vgoals,
                         const double *h_agoals, double *h_tau_ff, double *h_qdes, double *h_vdes,
                         double *h_f_with_delta, double *h_ddq_res, double *h_feet);
int qrw_wbc_get_stats(qrw_handle h, int32_t *h_iters, int32_t *h_status, double *h_rho, double *h_k_since_contact);
/* Scheduling only (no reference counterpart; results agree to rounding, ADMM iteration counts are identical): lanes per robot
 * instance of qrw_wbc_compute / qrw_wbc_compute_result.  16 (default): one 16-lane DPP row per instance, batch / 4 wavefronts --
 * 27.9 us per 4096 robots on the whole chip; 4: one quad per instance, batch / 16 wavefronts of 1.55 x the length -- 43.2 us on
 * the whole chip, but the faster one on a stream restricted to few compute units (the asynchronous control loop's 32).
 * QRW_WBC16=0 makes 4 the default of new handles. */
int qrw_wbc_set_lanes(qrw_handle h, int32_t lanes);

/* Stand-alone pieces of the WBC step with the reference's own signatures, for callers that
 * use the bound classes directly (scripts/solo12InvKin.py:62-67, scripts/QP_WBC.py:107-111):
 * InvKin::refreshAndCompute (+ get_q_step, get_dq_cmd): host arrays, batch of B.
 *   h_contacts [B][4], h_goals/vgoals/agoals [B][3][4], h_posf/vf/wf/af [B][4][3], h_Jf [B][12][12]
 *   -> h_ddq, h_dq_cmd, h_q_step [B][12] */
int qrw_invkin_host(qrw_handle h, const double *h_contacts, const double *h_goals, const double *h_vgoals,
                    const double *h_agoals, const double *h_posf, const double *h_vf, const double *h_wf,
                    const double *h_af, const double *h_Jf, double *h_ddq, double *h_dq_cmd, double *h_q_step);
/* QPWBC::run(M, Jc, f_cmd, RNEA, k_contacts) + get_f_res / get_ddq_res / get_H:
 *   h_M [B][18][18] (only the diagonal of its top-left 6x6 is read: the caller masks it,
 *   scripts/QP_WBC.py:93), h_Jc [B][12][18], h_f_cmd [B][12], h_RNEA [B][6]
 *   -> h_f_res [B][12], h_ddq_res [B][6], h_H [B][12][12] (may be NULL) */
int qrw_qpwbc_host(qrw_handle h, const double *h_M, const double *h_Jc, const double *h_f_cmd, const double *h_RNEA,
                   double *h_f_res, double *h_ddq_res, double *h_H);

/* Rigid-body slice used by Solo12InvKin (scripts/solo12InvKin.py:47-59): fixed-base feet
 * kinematics. h_q12/h_dq12 [B][12] -> h_posf/vf/wf/af [B][4][3], h_Jf [B][12][12] */
int qrw_fixed_feet_host(qrw_handle h, const double *h_q12, const double *h_dq12, double *h_posf, double *h_vf,
                        double *h_wf, double *h_af, double *h_Jf);

/* Diagonal of the neutral-configuration CRBA base block (scripts/QP_WBC.py:89-93), constant. */
int qrw_get_base_inertia_diag(qrw_handle h, double *h_Y6);

/* ---------------- planners feeding the hot path ----------------
 * Batched Gait + FootstepPlanner + FootTrajectoryGenerator + StatePlanner with persistent per-instance state,
 * wired as scripts/Controller.py:119-137 wires them. The timing parameters (dt_mpc, dt_wbc, T_gait, N_gait,
 * n_steps; T_mpc = n_steps * dt_mpc) come from the handle's qrw_config. */
typedef struct {
  int32_t k_mpc;            /* WBC iterations per MPC iteration (scripts/main_solo12_control.py:123)           */
  double h_ref;             /* StatePlanner::initialize h_ref_in, FootstepPlanner::initialize h_ref_in          */
  double shoulders[12];     /* 3x4 row-major, FootstepPlanner::initialize shouldersIn (Controller.py:131-135)    */
  double max_height;        /* FootTrajectoryGenerator::initialize maxHeightIn (Controller.py:137 -> 0.05)       */
  double lock_time;         /* ... lockTimeIn (0.07)                                                             */
  double init_target[12];   /* ... targetFootstepIn, 3x4                                                         */
  double init_foot_pos[12]; /* ... initialFootPosition, 3x4                                                      */
} qrw_planner_config;

/* Replaces Gait::initialize (src/Gait.cpp:19-36), StatePlanner::initialize (src/StatePlanner.cpp:12-19),
 * FootstepPlanner::initialize (src/FootstepPlanner.cpp:22-49), FootTrajectoryGenerator::initialize
 * (src/FootTrajectoryGenerator.cpp:22-38). Returns -3 where Gait::initialize throws (N_gait too small).
 *
 * The size rule. The gait matrices are 64-bit column masks (bit i = row i), so N_gait <= 63 (-1 otherwise), and -3 is returned,
 * before anything is launched, unless
 *     n_steps + 1 <= N_gait   and   rows_needed(T_gait, dt_mpc) <= N_gait,
 *     rows_needed = max(2 lround(0.5 T_gait / dt_mpc), 4 lround(0.25 T_gait / dt_mpc), lround(T_gait / dt_mpc)):
 * the rows the pacing / bounding / trot generators, the walk generator and the static generator write. Gait::initialize tests
 * the last of the three only (src/Gait.cpp:30-31) and a joystick code then writes outside the matrices when another is larger.
 * A period that fills the table exactly (rows_needed == N_gait) is legal and means "row N_gait counts as a zero row"; the
 * reference reads past its matrices there. A refused handle stays uninitialised: its planner calls return -1.
 * qrw_gait_table_fits asks that rule (with N_gait <= 63) of a handle's configuration without initialising or launching
 * anything: 1 fits, 0 qrw_planner_init would refuse, -1 null handle. */
int qrw_planner_init(qrw_handle h, const qrw_planner_config *pc, void *stream);
int qrw_gait_table_fits(qrw_handle h);

/* One control iteration of the planners, in the order of scripts/Controller.py:222-236:
 * Gait::updateGait(k, k_mpc, q, code) (src/Gait.cpp:184-192), FootstepPlanner::updateFootsteps(k % k_mpc == 0 && k != 0,
 * k_mpc - k % k_mpc, q, b_v, b_vref) (src/FootstepPlanner.cpp:51), FootTrajectoryGenerator::update(k, o_target)
 * (src/FootTrajectoryGenerator.cpp:108), StatePlanner::computeReferenceStates(q, v, vref, 0) (src/StatePlanner.cpp:21).
 *   in : d_q7 [B][q_ld] of which the first 7 entries of a row are read (position, quaternion xyzw; q_ld = 7, or 19 to
 *        pass the q [B][19] of qrw_controller_update_state directly), d_hv [B][6], d_vref [B][6], d_code [B] int32
 *        joystick codes or NULL (code_scalar then applies; 1 pacing, 2 bounding, 3 trot, 4 static as
 *        src/Gait.cpp:194-219; 5 walk)
 *   out: d_xref [B][12][N+1], d_fsteps [B][N_gait][12], d_gait [B][N_gait][4] (current gait), d_target [B][3][4]
 *        (o_targetFootstep), d_feet_pva [B][3][3][4] (foot position, velocity, acceleration goals), d_contacts [B][4]
 *        (row 0 of the current gait = the `contacts` operand of qrw_wbc_compute); any may be NULL */
int qrw_planner_step(qrw_handle h, int32_t k, const double *d_q7, int32_t q_ld, const double *d_hv, const double *d_vref,
                     const int32_t *d_code, int32_t code_scalar, double *d_xref, double *d_fsteps, double *d_gait,
                     double *d_target, double *d_feet_pva, double *d_contacts, void *stream);

/* One planner method at a time with host buffers (backs the bound-class drop-ins Gait / FootstepPlanner /
 * FootTrajectoryGenerator / StatePlanner, python/gepadd.cpp:44-181). mode is a bit set: 2 Gait::updateGait,
 * 4 FootstepPlanner::updateFootsteps (k_footsteps, refresh), 8 FootTrajectoryGenerator::update (h_target_in or the stored
 * target), 16 StatePlanner::computeReferenceStates (z_average), 32 only copy the requested outputs. */
int qrw_planner_call_host(qrw_handle h, int32_t mode, int32_t k, int32_t k_footsteps, int32_t refresh, const double *h_q7,
                          const double *h_v6, const double *h_vref6, int32_t code, const double *h_target_in,
                          double z_average, double *h_xref, double *h_fsteps, double *h_gait, double *h_target,
                          double *h_feet_pva);

/* Getter of planner state items of instance b (count doubles): which = 0 past gait, 1 current gait, 2 desired gait
 * (N_gait*4 each), 3 newPhase, 4 is_static, 5 remainingTime, 6 #swing feet, 7 targetFootstep (12), 8 o_targetFootstep (12),
 * 9/10/11 foot position/velocity/acceleration (12), 12 t0s (4), 13 t_swing (4), 14 footsteps (N_gait*12, [row][xyz][foot]),
 * 15 currentFootstep (12), 16 q_static (7), 17 trajectory target (12). */
int qrw_planner_get_host(qrw_handle h, int32_t which, int32_t b, int32_t count, double *h_out);

/* ---------------- controller glue around the hot path ----------------
 * The element-wise parts of Controller.compute (scripts/Controller.py) between planners, MPC and WBC, batched, with
 * their per-instance state (perfect x/y/yaw integration, previous foot commands, previous q_des / v_des, error flag). */
/* Controller.__init__ state (scripts/Controller.py:119-123,154): d_q_init12 [B][12] (or NULL = zeros) -> qdes[7:]. */
int qrw_controller_init(qrw_handle h, const double *d_q_init12, double h_ref, void *stream);
/* Controller.updateState (scripts/Controller.py:381-426, non-static branch): d_joy_vref [B][6], d_q_filt [B][19],
 * d_v_filt [B][18], d_rpy [B][3] -> d_q [B][19], d_v [B][18], d_hv [B][6], d_vref [B][6] (may be NULL),
 * d_oRh_oTh [B][12] = oRh row-major | oTh (may be NULL). */
int qrw_controller_update_state(qrw_handle h, const double *d_joy_vref, const double *d_q_filt, const double *d_v_filt,
                                const double *d_rpy, double *d_q, double *d_v, double *d_hv, double *d_vref,
                                double *d_oRh_oTh, void *stream);
/* WBC target assembly (scripts/Controller.py:258-296): d_x_f_mpc [B][24][N], d_xref [B][12][N+1], d_feet_pva [B][3][3][4]
 * (FootTrajectoryGenerator position / velocity / acceleration), d_v [B][18] -> d_x_f_wbc [B][24] (may be NULL),
 * d_q_wbc [B][19], d_b_v [B][18], d_f_cmd [B][12] (= x_f_wbc[12:], may be NULL), d_feet_cmd [3][B][3][4] (planes feet_p_cmd, feet_v_cmd, feet_a_cmd,
 * each directly usable as the pgoals / vgoals / agoals operand of qrw_wbc_compute). */
int qrw_controller_wbc_inputs(qrw_handle h, const double *d_x_f_mpc, const double *d_xref, const double *d_feet_pva,
                              const double *d_v, double *d_x_f_wbc, double *d_q_wbc, double *d_b_v, double *d_f_cmd,
                              double *d_feet_cmd, void *stream);
/* Result + security_check (scripts/Controller.py:306-310,341-365): d_tau_ff [B][12], d_qdes [B][19], d_vdes [B][18],
 * d_q_filt [B][19], d_v_secu [B][12] -> d_result [B][5][12] = P, D, q_des, v_des, tau_ff (0.8 x), d_error_flag [B]
 * int32 (0 ok, 1 joint position, 2 joint velocity, 3 torque: the reference's three codes; 4: a non-finite tau_ff / q_des /
 * v_des -- NOT in the reference, whose `> limit` comparisons are blind to NaN and would pass it to the motors; sticky, may be
 * NULL).  Any code sets the reference's security output (P = 0, D = 0.1, zero targets and torques). */
int qrw_controller_result(qrw_handle h, const double *d_tau_ff, const double *d_qdes, const double *d_vdes,
                          const double *d_q_filt, const double *d_v_secu, double *d_result, int32_t *d_error_flag,
                          void *stream);

/* Bookkeeping of MPC_Wrapper.solve on the result the loop currently reads (scripts/MPC_Wrapper.py:89-102; observable in
 * the reference's asynchronous mode only, where get_latest_result keeps returning it until the child process delivers):
 * rows 12..23 of d_x_f_mpc [B][24][N] are rolled one column to the left (np.roll, the first column wraps to the end) and,
 * when the last non-zero row of d_gait [B][N_gait][4] differs from row 0, the last column becomes m g / n_contacts
 * (mass 2.5) on that row's stance feet.  The caller applies it when k > 2 (:89), as the reference does. */
int qrw_mpc_result_shift(qrw_handle h, const double *d_gait, double *d_x_f_mpc, void *stream);

/* Fused forms of the above, one launch each, for the device-resident control loop (same arithmetic):
 * qrw_control_pre = qrw_controller_update_state + qrw_planner_step (fed with its q, h_v, v_ref) and, when d_x_f_mpc is
 * not NULL (the MPC result to use is already known: every iteration that does not solve), + qrw_controller_wbc_inputs;
 * qrw_wbc_compute_result = qrw_wbc_compute + qrw_controller_result (scripts/Controller.py:200-326 end to end in two
 * launches plus the MPC solve every k_mpc-th iteration).  Operands as in the separate entry points.  d_fsteps and d_gait may
 * be NULL; with d_fsteps NULL and d_x_f_mpc given (an iteration that does not solve: nobody reads the MPC's inputs) only
 * column 0 and horizon step 1 of d_xref are written, which is all the WBC target assembly reads of it, and of the planner's
 * own copy of the footstep table (qrw_planner_get item "fsteps") only rows 0 and 1 are refreshed -- row 1 is what
 * updateNewContact may take at the next gait change (src/FootstepPlanner.cpp:225-230), the other rows are rewritten by the
 * next call with d_fsteps before anything reads them. */
int qrw_control_pre(qrw_handle h, int32_t k, const double *d_joy_vref, const double *d_q_filt, const double *d_v_filt,
                    const double *d_rpy, const int32_t *d_code, int32_t code_scalar, const double *d_x_f_mpc, double *d_q,
                    double *d_v, double *d_hv, double *d_vref, double *d_oRh_oTh, double *d_xref, double *d_fsteps,
                    double *d_gait, double *d_target, double *d_feet_pva, double *d_contacts, double *d_x_f_wbc,
                    double *d_q_wbc, double *d_b_v, double *d_f_cmd, double *d_feet_cmd, void *stream);
int qrw_wbc_compute_result(qrw_handle h, const double *d_q, const double *d_dq, const double *d_f_cmd,
                           const double *d_contacts, const double *d_pgoals, const double *d_vgoals,
                           const double *d_agoals, double *d_tau_ff, double *d_qdes, double *d_vdes,
                           double *d_f_with_delta, double *d_ddq_res, double *d_feet, const double *d_q_filt,
                           const double *d_v_secu, double *d_result, int32_t *d_error_flag, void *stream);

/* A control iteration that does not solve (qrw_control_pre given d_x_f_mpc, without d_fsteps / d_gait, + qrw_wbc_compute_result
 * on its outputs) with every buffer BOUND ONCE: a control loop passes the same buffers on every tick -- the sensor values are
 * written into fixed input arrays, the outputs read from fixed ones -- so the ~50 pointer arguments of the two calls need not be
 * marshalled again every 2 ms (scripts/Controller.py:200-326 runs 9 of 10 iterations this way, :246).  qrw_iteration_bind stores
 * the pointers in the handle (no launch, no allocation; binding again replaces them); qrw_iteration_step enqueues the two launches
 * for iteration k on `stream` using the MPC result d_x_f_mpc [B][24][N] (whichever buffer the loop has adopted).  Same kernels,
 * same arithmetic as the two separate calls.  Why not a HIP graph: on this runtime hipGraphLaunch of the captured pair costs
 * 19 us of host time against 8.6-9.3 us for the two launches (scripts/ubench/graph_launch.hip, profiles/r5_graph_launch.txt). */
typedef struct {
  /* inputs (read every step) */
  const double *d_joy_vref, *d_q_filt, *d_v_filt, *d_rpy, *d_v_secu;
  const int32_t *d_code; /* per-robot joystick codes or NULL */
  int32_t code_scalar;   /* used when d_code is NULL         */
  /* outputs of qrw_control_pre (d_fsteps / d_gait are not produced on an iteration that does not solve) */
  double *d_q, *d_v, *d_hv, *d_vref, *d_oRh_oTh, *d_xref, *d_target, *d_feet_pva, *d_contacts, *d_x_f_wbc, *d_q_wbc, *d_b_v,
      *d_f_cmd, *d_feet_cmd;
  /* outputs of qrw_wbc_compute_result */
  double *d_tau_ff, *d_qdes, *d_vdes, *d_f_with_delta, *d_ddq_res, *d_feet, *d_result;
  int32_t *d_error_flag;
} qrw_iteration_buffers;
int qrw_iteration_bind(qrw_handle h, const qrw_iteration_buffers *buffers);
int qrw_iteration_step(qrw_handle h, int32_t k, const double *d_x_f_mpc, void *stream);

/* ---------------- state estimator: sensors in, filtered state out ----------------
 * The stage of Controller.compute before everything above (scripts/Controller.py:213): Estimator.run_filter
 * (scripts/Estimator.py:466-629), batched, with its per-instance state (contact counters, the filters, yaw offset, call counter)
 * in the handle.  Both of the reference's filters for base position and velocity are provided, chosen by how the handle's
 * estimator was last initialised: the cascade of complementary filters (qrw_estimator_init: kf_enabled = False, as
 * scripts/Controller.py:110-111 builds it) and the Kalman filter over base position, base velocity and the four foot positions
 * (qrw_estimator_init_kalman: KFilterBis, kf_enabled = True, :88-181 and :555-580).  Everything else of run_filter is common to
 * the two.  The outputs are the d_q_filt / d_v_filt / d_rpy / d_v_secu operands of qrw_controller_update_state, qrw_control_pre
 * and qrw_iteration_bind: a sensors-in iteration is qrw_estimator_step writing into those buffers, followed by
 * qrw_iteration_step or qrw_control_pre on the same stream.  Not provided: KFilter (the 6-state class that Estimator never
 * constructs), the logging arrays, plot_graphs.  One departure: the scan for `remaining_steps` (:476-479) stops at N_gait where
 * the reference raises IndexError (every row equal to row 0). */
typedef struct {
  double h_init;   /* initial base height: FK_xyz[2] and the position filter's low-pass state (scripts/Estimator.py:279-283) */
  int32_t perfect; /* perfectEstimator (:595-596, :601-602): base height and base-frame velocity taken from the true inputs   */
} qrw_estimator_config;

/* Replaces Estimator.__init__ (scripts/Estimator.py:245-342) with kf_enabled = False; dt is the handle's dt_wbc.  Resets the
 * state: calling it again re-initialises (the yaw offset is latched again by the next two steps), and switches a handle that
 * was in Kalman mode back to the complementary filters: after it the handle's estimator is that of a fresh handle. */
int qrw_estimator_init(qrw_handle h, const qrw_estimator_config *cfg, void *stream);

/* The tuning values of the Kalman filter (scripts/Estimator.py:133-137; the reference's values: 0.1, 1.0, 0.1, 0.1, 30). */
typedef struct {
  double sigma_kin; /* kinematic measurement noise: R = sigma_kin^2 / trust on a foot's three rows                        */
  double sigma_h;   /* foot height measurement noise: R = sigma_h^2 / trust on row 12 + foot                              */
  double sigma_a;   /* acceleration noise: Q = sigma_a^2 dt^2 on the velocity states                                      */
  double sigma_dp;  /* foot slip: Q = sigma_dp^2 (1 + exp(gamma (0.5 - trust))) dt^2 on a foot's states                   */
  double gamma;     /* trust = 1 for a foot in stance, 0.01 in swing                                                      */
} qrw_kalman_config;

/* The same with kf_enabled = True: resets the shared state exactly as qrw_estimator_init does (except that the base height
 * goes into X[2], not into the position filter, :282-285), sets X = 0 but X[2] = h_init and P = I (:121), and switches the
 * handle's estimator to the Kalman filter; qrw_estimator_step / _step_host then run that.  kcfg NULL = the reference's values;
 * the sigmas must be > 0 and finite, gamma finite.  The first call on a handle allocates the filter's state (142 doubles per
 * instance: X, the three per-axis 6x6 blocks of P, the last Z), which stays with the handle until qrw_destroy and which
 * qrw_state_bytes counts from then on; a handle that never calls it allocates nothing for it. */
int qrw_estimator_init_kalman(qrw_handle h, const qrw_estimator_config *cfg, const qrw_kalman_config *kcfg, void *stream);

/* Replaces Estimator.run_filter(k, gait, device, goals) (scripts/Estimator.py:466-629).  Only enqueues: no allocation, no
 * synchronisation.
 *   in : d_lin_acc [B][3] (device.baseLinearAcceleration), d_ang_vel [B][3] (baseAngularVelocity), d_quat [B][4] xyzw
 *        (baseOrientation), d_q_mes [B][12], d_v_mes [B][12];
 *        d_gait [B][N_gait][4] or NULL = the current gait of the handle's planner; d_goals [B][3][4] or NULL = its
 *        FootTrajectoryGenerator::getFootPosition (item 9 of qrw_planner_get_host) -- NULL needs qrw_planner_init;
 *        d_true_pos [B][3] (device.dummyPos) and d_true_b_vel [B][3] (device.b_baseVel): both given when the estimator was
 *        initialised with perfect != 0, both NULL otherwise
 *   out: d_q_filt [B][19], d_v_filt [B][18], d_rpy [B][3] (Estimator.RPY, yaw offset removed), d_v_secu [B][12] */
int qrw_estimator_step(qrw_handle h, const double *d_lin_acc, const double *d_ang_vel, const double *d_quat,
                       const double *d_q_mes, const double *d_v_mes, const double *d_gait, const double *d_goals,
                       const double *d_true_pos, const double *d_true_b_vel, double *d_q_filt, double *d_v_filt,
                       double *d_rpy, double *d_v_secu, void *stream);
/* The same with host buffers, synchronised per handle (backs the single-robot drop-in Estimator.py). */
int qrw_estimator_step_host(qrw_handle h, const double *h_lin_acc, const double *h_ang_vel, const double *h_quat,
                            const double *h_q_mes, const double *h_v_mes, const double *h_gait, const double *h_goals,
                            const double *h_true_pos, const double *h_true_b_vel, double *h_q_filt, double *h_v_filt,
                            double *h_rpy, double *h_v_secu);

/* Getter of estimator state items of instance b (count doubles): which = 0 k_since_contact (4), 1 FK_lin_vel (3), 2 FK_xyz (3),
 * 3 xyz_mean_feet (3), 4 / 5 filter_xyz_vel HP_x / LP_x (3), 6 / 7 filter_xyz_pos HP_x / LP_x (3), 8 alpha, 9 close_from_contact,
 * 10 offset_yaw_IMU, 11 k_log, 12 filt_lin_vel (3). */
int qrw_estimator_get_host(qrw_handle h, int32_t which, int32_t b, int32_t count, double *h_out);
/* ... of the Kalman filter's: which = 0 X (18), 1 P (324: row-major 18 x 18, assembled from the per-axis blocks, exact zeros
 * between the axes), 2 Z (16, the last measurement).  -1 "not in Kalman mode" unless the estimator was last initialised by
 * qrw_estimator_init_kalman.  (The items of qrw_estimator_get_host stay available; the complementary filters' halves keep
 * their initial values in Kalman mode, as in the reference.) */
int qrw_estimator_kalman_get_host(qrw_handle h, int32_t which, int32_t b, int32_t count, double *h_out);

/* ---------------- rigid-body simulator: torques in, sensor readings out ----------------
 * What closes the loop around the controller: per instance one Solo12 on a flat plane, stepped on the device.  One tick is the
 * reference's SendCommand followed by the next UpdateMeasurment (scripts/PyBulletSimulator.py:672-710, :588-633): the PD+ law
 * tau = tau_ff + P (q_des - q) + D (v_des - dq) from the joint state at the start of the tick, held over `substeps` semi-implicit
 * Euler steps of the forward dynamics, then the readings qrw_estimator_step takes, in its layouts.  The physics is NOT
 * PyBullet's: penalty contact (fn = max(0, kn d - dn vz) while the penetration d = foot_radius - z_foot > 0, friction
 * -mu fn v_t / sqrt(|v_t|^2 + vs^2)) on the plane z = 0, or on a heightfield (qrw_sim_set_terrain below); no joint limits, no
 * joint friction, no motor model.
 * State per instance, QRW_SIM_STATE_ITEMS doubles: q19 (position, quaternion xyzw, joints FL FR HL HR), v18 (base linear and
 * angular velocity in the base frame, joint velocities), prev_o_imuVel (3), tick counter, status.  A robot whose new state is not
 * finite gets status 1 and is frozen: nothing of that tick or a later one is stored for it (its rows of the output buffers keep
 * what the last finite tick wrote); the others are unaffected. */
#define QRW_SIM_STATE_ITEMS 42
typedef struct {
  double dt;           /* tick (0.002, the controller's dt_wbc)                                  */
  int32_t substeps;    /* >= 1 (8)                                                               */
  double kn, dn;       /* normal stiffness N/m (1e4) and damping N s/m (60)                      */
  double mu, vs;       /* friction coefficient (0.9) and regularisation velocity m/s (0.01)      */
  double foot_radius;  /* 0.0155 (scripts/Estimator.py:596)                                      */
  double base_height;  /* base height of qrw_sim_init with q_ld = 12 (0.2596: feet resting at 0.7 / -1.4) */
} qrw_sim_params;
/* device output buffers of a tick: the first five are the inputs of qrw_estimator_step, d_true_pos / d_true_b_vel those of a
 * perfect estimator (dummyPos, b_baseVel); d_o_imu_vel is o_imuVel, d_contact_forces the world forces on the feet in the last
 * sub-step, d_joint_torques the tick's tau.  None may be NULL. */
typedef struct {
  double *d_q_mes, *d_v_mes;      /* [B][12] */
  double *d_quat;                 /* [B][4] xyzw */
  double *d_ang_vel, *d_lin_acc;  /* [B][3] base frame (baseAngularVelocity, baseLinearAcceleration) */
  double *d_o_imu_vel, *d_true_pos, *d_true_b_vel; /* [B][3] */
  double *d_contact_forces;       /* [B][4][3] */
  double *d_joint_torques;        /* [B][12] */
} qrw_sim_buffers;

/* Sets the state (d_q_init [B][q_ld]: q_ld = 19 the whole q19, q_ld = 12 the joints with the base level at params->base_height
 * (above the highest ground under its feet when a terrain is set);
 * velocities, prev_o_imuVel, tick and status zero) and writes the first measurement, as the reference's first UpdateMeasurment.
 * Again = re-initialise: every robot whose d_q_init is finite starts afresh with status 0, whatever its status was.  A robot
 * whose d_q_init is not finite gets status 1 and nothing else of it is stored: its other state items and its rows of the output
 * buffers keep what they held (the state zero in a handle that was never initialised before); the others are unaffected. */
int qrw_sim_init(qrw_handle h, const double *d_q_init, int32_t q_ld, const qrw_sim_params *params, const qrw_sim_buffers *out,
                 void *stream);
/* One tick.  d_P, d_D, d_q_des, d_v_des, d_tau_ff: rows of 12 per instance, cmd_ld doubles apart (12 for five plain [B][12]
 * buffers, 60 for the five planes of a qrw_controller_result [B][5][12]); d_f_ext [B][6] a world force and moment at the base
 * origin, or NULL.  Only enqueues. */
int qrw_sim_step(qrw_handle h, const double *d_P, const double *d_D, const double *d_q_des, const double *d_v_des,
                 const double *d_tau_ff, int32_t cmd_ld, const double *d_f_ext, const qrw_sim_buffers *out, void *stream);
/* The same two with host buffers ([B][q_ld] initial configuration, [B][12] commands, h_f_ext [B][6] or NULL; h_out holds HOST
 * pointers, NULL = not wanted), synchronised per handle (they back the single-robot drop-in PyBulletSimulator.py).  The
 * measurements live in device buffers the handle allocates at the first qrw_sim_init_host; qrw_sim_step_host needs that call. */
int qrw_sim_init_host(qrw_handle h, const double *h_q_init, int32_t q_ld, const qrw_sim_params *params, const qrw_sim_buffers *h_out);
int qrw_sim_step_host(qrw_handle h, const double *h_P, const double *h_D, const double *h_q_des, const double *h_v_des,
                      const double *h_tau_ff, const double *h_f_ext, const qrw_sim_buffers *h_out);
/* The whole state, [QRW_SIM_STATE_ITEMS][batch] (item-major, as the device holds it): for tests and restarts.  Setting it does
 * not rewrite the measurement buffers.  A frozen robot given a finite state and status 0 steps again from the next tick on. */
int qrw_sim_get_host(qrw_handle h, double *h_state);
int qrw_sim_set_host(qrw_handle h, const double *h_state);

/* Heightfield terrain instead of the plane z = 0: ONE field per handle, shared by all its robots.  Heights [rows][cols] in C
 * order, rows, cols >= 2; vertex (r, c) lies at world x = x0 + c dx, y = y0 + r dy (dx, dy > 0).  Every cell is cut by the diagonal
 * from (r, c) to (r+1, c+1) and a foot is in contact with the plane of the triangle under it: with its unit normal n,
 * d = foot_radius - n_z (z_foot - h), normal force kn d - dn (n.v) clipped at 0 while d > 0, friction against the tangential
 * velocity as on the plane (a field of zeros IS the plane's formula).  d_origin_xy [B][2], or NULL: robot b's feet at world
 * (x, y) are looked up at (x + ox[b], y + oy[b]), so that every robot can walk a patch of its own.  Outside the field the
 * surface continues as the clamped point of the edge cell (unphysical; never a fault, whatever the coordinate).
 * The handle keeps a copy of its own (device-to-device on `stream`, ordered like a tick; reallocated only when the size
 * changes).  The setting survives qrw_sim_init; qrw_sim_init with q_ld = 12 then puts the level base at (0, 0) base_height above
 * the highest ground under its four feet.  Refused (-1): rows or cols < 2, a spacing that is not positive and finite, NULL
 * heights.  _host: the same from host pointers, synchronised per handle.  qrw_sim_clear_terrain: back to the plane. */
int qrw_sim_set_terrain(qrw_handle h, const double *d_heights, int32_t rows, int32_t cols, double x0, double y0, double dx,
                        double dy, const double *d_origin_xy, void *stream);
int qrw_sim_set_terrain_host(qrw_handle h, const double *h_heights, int32_t rows, int32_t cols, double x0, double y0, double dx,
                             double dy, const double *h_origin_xy);
int qrw_sim_clear_terrain(qrw_handle h);

/* ---------------- joystick: the tick in, reference velocity, gait code and push out ----------------
 * The first line of the reference's control iteration, Joystick.update_v_ref(k, velID) (scripts/Controller.py:210), as a device
 * stage with per-robot scenarios: its outputs are the d_joy_vref operand of qrw_controller_update_state / qrw_control_pre /
 * qrw_iteration_bind, the d_code operand of the planners and the d_f_ext operand of qrw_sim_step.  Stateless in the tick: but for
 * the gamepad filter and the stop latch every output is a function of k and the tables alone.  The velocity comes from ONE of
 *   QRW_JOY_PROFILE  handle_v_switch / apply_velocity_change (scripts/Joystick.py:160-190): cubic blends between the columns of a
 *                    per-robot switch table; after the last switch the value of the tick before it is held, as the reference does;
 *   QRW_JOY_RAMP     update_v_ref_multi_simu (:289-315): (Vx, Vy, Vw) ramped from tick k_start over beta = (int) max(|V| 10000,
 *                    100) ticks (2500 for Vw);
 *   QRW_JOY_GAMEPAD  the low-pass filter of update_v_ref_gamepad with its dead band (:135-137) on the command given to every step;
 * the codes are computeCode's one-shot (:144-158) from a schedule of (tick, code) pairs -- `code` on that tick, 0 on every other,
 * the later pair wins on equal ticks -- and the pushes are apply_external_force (scripts/PyBulletSimulator.py:402-431): the sum, in
 * table order, of alpha [F; M] over the entries with start <= k <= start + duration.  Departure: that wrench is the simulator's
 * world wrench at the base origin, not Bullet's LINK_FRAME.  Not provided: the gamepad client, the `reduced` flag, joystick.stop
 * reaching the controller's security branch, the velID tables (callers pass their own).
 * Limits (the integer powers of the polynomials must be exact in a double): two consecutive switches are at most 2^17 ticks apart,
 * k_switch is non-decreasing and starts at or before tick 0, a push lasts 1 .. 2^13 ticks, |V| 10000 < 2^31; ticks are >= 0.
 * A table shorter than the fleet's common length is padded: a profile by repeating its last column, the codes with a negative
 * tick, the pushes with a window before tick 0 -- none of which changes a bit of the outputs. */
#define QRW_JOY_PROFILE 0
#define QRW_JOY_RAMP 1
#define QRW_JOY_GAMEPAD 2
typedef struct {
  int32_t mode;       /* QRW_JOY_PROFILE, QRW_JOY_RAMP or QRW_JOY_GAMEPAD                                          */
  int32_t n_switch;   /* profile: columns per robot, 1..32 (1: zeros)                                              */
  int32_t n_codes;    /* (tick, code) pairs per robot, 0..16                                                       */
  int32_t n_pushes;   /* pushes per robot, 0..8                                                                    */
  int32_t k_start;    /* ramp: first tick of the ramps (the reference's k_mpc * 16 * 3)                            */
  double gp_alpha;    /* gamepad: filter coefficient in (0, 1]; the reference's is the quotient 0.0020 / 0.02      */
  double gp_deadband; /* gamepad: components with -band < v < band become 0; >= 0, the reference's is 0.005        */
} qrw_joystick_config;
/* HOST pointers, robot-major (what a caller writes down per robot); a table its mode or its count does not use may be NULL */
typedef struct {
  const int32_t *k_switch;   /* [B][n_switch]                      */
  const double *v_switch;    /* [B][6][n_switch]                   */
  const double *ramp_v;      /* [B][3] Vx, Vy, Vw                  */
  const int32_t *code_k;     /* [B][n_codes] ticks                 */
  const int32_t *code_v;     /* [B][n_codes] codes                 */
  const int32_t *push_k;     /* [B][n_pushes][2] start, duration   */
  const double *push_w;      /* [B][n_pushes][6] F (3), M (3)      */
} qrw_joystick_tables;
/* Replaces Joystick.__init__ (scripts/Joystick.py:14-58) and update_for_analysis (:317-326) / the tables of
 * update_v_ref_predefined (:201-284).  A set-up call: the tables are validated on the host before anything is launched (-1, with
 * the offending robot and entry in qrw_last_error(); the handle keeps what it had), the handle owns device copies (item-major),
 * and the state -- the filter's v_ref zero, k_stop -1 -- is written by a launch on `stream`.  Synchronised per handle (state family
 * "joystick").  Again = re-initialise: afterwards the state is a fresh handle's, bit for bit.  The first call allocates the state
 * (7 doubles per robot), which qrw_state_bytes counts from then on; a handle that never calls it allocates nothing. */
int qrw_joystick_init(qrw_handle h, const qrw_joystick_config *cfg, const qrw_joystick_tables *tables, void *stream);
/* Replaces Joystick.update_v_ref(k, velID) (scripts/Joystick.py:60-79) and the apply_external_force calls of a tick
 * (scripts/PyBulletSimulator.py:354-356) for tick k >= 0.  Only enqueues.
 *   in : d_v_gp [B][6] this tick's unfiltered command: required in gamepad mode, NULL otherwise; d_stop [B] int32 or NULL (in a
 *        fleet the controller's d_error_flag): the first tick on which d_stop[b] != 0 becomes the robot's k_stop, and from that
 *        tick on its three outputs are zero and its filter state is frozen, also when the flag is cleared again (the reference
 *        leaves its loop at the first error, scripts/main_solo12_control.py:180)
 *   out: d_joy_vref [B][6]; d_code [B] int32 or NULL; d_f_ext [B][6]: required when the handle has pushes (zeros while none is
 *        active), optional (zeros) otherwise */
int qrw_joystick_step(qrw_handle h, int32_t k, const double *d_v_gp, const int32_t *d_stop, double *d_joy_vref, int32_t *d_code,
                      double *d_f_ext, void *stream);
/* The same with host buffers, synchronised per handle. */
int qrw_joystick_step_host(qrw_handle h, int32_t k, const double *h_v_gp, const int32_t *h_stop, double *h_joy_vref,
                           int32_t *h_code, double *h_f_ext);
/* Getter of the joystick state (the reference's Joystick.v_ref in gamepad mode; the outcome `finished` of control_loop,
 * scripts/main_solo12_control.py:180,239, per robot): which = 0 the filter's v_ref of robot b (count <= 6 doubles), 1 k_stop of
 * the robots b .. b + count - 1 (-1: never stopped). */
int qrw_joystick_get_host(qrw_handle h, int32_t which, int32_t b, int32_t count, double *h_out);

/* ---------------- asynchronous MPC ----------------
 * The reference runs the MPC in a child process on its own CPU core and polls a shared flag
 * (scripts/MPC_Wrapper.py:150-298).  Here the MPC gets its own HIP stream restricted to a subset of the compute
 * units, so that the control loop's kernels (planners, WBC, glue) on a second stream restricted to the remaining
 * units never queue behind a running solve.  Creates a stream whose kernels only run on compute units
 * [first_cu, first_cu + n_cus) of `device` (hipExtStreamCreateWithCUMask); n_cus <= 0 = no restriction. */
int qrw_stream_create(int32_t device, int32_t first_cu, int32_t n_cus, void **stream);
int qrw_stream_destroy(void *stream);
/* number of compute units of the device (256 on MI355X) */
int qrw_device_cu_count(int32_t device, int32_t *n_cus);
/* Stream hand-over without host synchronisation: everything enqueued on `waiter` after this call runs after what is on `signaller`
 * now (hipEventRecord on `signaller` + hipStreamWaitEvent on `waiter`, with an event the handle keeps: two runtime calls, where
 * torch's Stream.wait_stream creates and destroys an event object each time -- ~12 us, and a joined stream-group iteration needs
 * several).  Plumbing of the stream-group / asynchronous modes; no reference counterpart (a child process and flags there). */
int qrw_stream_wait_stream(qrw_handle h, void *waiter, void *signaller);

/* Diagnostic: checks on the device what the MPC solver's linear algebra relies on — the row_newbcast form of
 * v_fmac_f64, the twisted block sweeps in the production LDS layout and the in-register Gauss-Jordan inverse
 * (csrc/chain_sweep.h) — against a host evaluation — and then one whole known-answer MPC solve (the reference's
 * four-stance immobile scenario, scripts/test_mpc.py:54-62: 350 ADMM iterations, equal vertical forces, see
 * csrc/qrw_selftest.hip).  0 = ok, 1 = sweep mismatch, 2 = the known-answer solve is wrong, <0 = HIP error. *max_err (of the
 * sweep check) may be NULL.  qrw_create runs the known-answer solve once per process and device and fails with -20 if
 * this build of the library computes wrong results (docs/HISTORY.md 6b). */
int qrw_selftest_sweeps(double *max_err);

/* workspace sizes, for callers that budget HBM */
int64_t qrw_state_bytes(qrw_handle h);

#ifdef __cplusplus
}
#endif
#endif /* QRW_HIP_H_ */

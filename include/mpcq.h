/* mpcq.h — C ABI of libmpcq.so, the MI355X (gfx950) batched MPC+RGP control-step engine.
 *
 * Drop-in boundary.  In the reference the hot path sits behind the Python class
 * `quad_optimizer` (src/quad_opt.py:35) whose only native FFI is acados_template's ctypes binding
 * of the generated solver: `.set(stage,'yref'|'lbx'|'ubx'|'p',…)`, `.solve()`, `.get(stage,'x'|'u')`,
 * `.get_stats('time_tot')`, `.get_cost()` (src/quad_opt.py:286-290,311-315,328-333,342-350,404),
 * plus numpy code for the recursive GP (src/gp/RGP.py:303-330 through src/gp/GPE.py:244-268).
 * This header is the batched analogue: one engine = B independent quadrotors advanced in lockstep,
 * all state (SQP iterate, RGP mean/covariance, trajectory cursor) resident in HBM between calls.
 *
 * Conventions: every function returns 0 on success and a negative mpcq_status on failure
 * (mpcq_last_error() gives the message).  All host arrays are caller-owned, C-contiguous,
 * float64, batch-major [B, ...] exactly like the numpy arrays of the reference facade; the
 * engine converts to its compute precision on the device.  Calls block until the result is
 * available unless the name ends in _async.  Not thread-safe per handle (the reference drives
 * its solver from one rospy callback thread, src/mpc_controller_node.py:234).
 *
 * State layout: x = [p(3), q = (w,x,y,z)(4), v(3) world, r(3) body]  (src/quad_opt.py:168-174),
 * u in [0,1]^4 (src/quad_opt.py:142-144), y = [x, u] (17).
 */
#ifndef MPCQ_H
#define MPCQ_H

#include <stdint.h>
#include "mpcq_nl_options.h"   /* mpcq_minsnap_nl_options (mpcq_replan_nonlinear) */

#ifdef __cplusplus
extern "C" {
#endif

#define MPCQ_NX 13
#define MPCQ_NU 4
#define MPCQ_NY 17

typedef enum mpcq_status {
  MPCQ_OK = 0,
  MPCQ_ERR_INVALID = -1,   /* bad argument / configuration */
  MPCQ_ERR_DEVICE = -2,    /* HIP runtime error (no GPU, OOM, launch failure) */
  MPCQ_ERR_STATE = -3,     /* call sequence error (e.g. step before set_trajectories) */
  MPCQ_ERR_COMM = -4       /* RCCL error */
} mpcq_status;

/* per-instance solver status, the acados return codes the reference discards (src/quad_opt.py:333) */
#define MPCQ_SOLVE_OK 0
#define MPCQ_SOLVE_NAN 1          /* the QP step was not finite: the instance kept its previous iterate and control */
#define MPCQ_SOLVE_MAXITER 2
#define MPCQ_SOLVE_QP_FAILURE 4
#define MPCQ_SOLVE_LOW_ACCURACY 8 /* MPCQ_PRECISION_F32 only, a warning: the step was taken, but its control may be off by more than the 1e-4 budget.
                                     Either the refinement of the QP solution against fp64 residuals did not converge (the step is the
                                     interior point's float answer), or the working set cycled under the float factorisation and the set the
                                     method settled on ignores a wrong-signed multiplier worth more than 1e-6 of a control (round 6; until then
                                     such solves came back with status 0, up to 0.43 of full thrust off on a flight that tumbles).  One in 7 M
                                     solves of the bench workload checked against the fp64 engine, on a quadrotor that is lost (QP gradient
                                     scale 1e9; DESIGN.md section 3.2, INTEGRATION.md says the same): expected where a flight is lost
                                     altogether.  Every solve that reports 0 is within the
                                     budget (tests/parity_cases.py: case_f32_every_solve_against_f64).  Not a failure:
                                     mpcq_get_tracking_stats out[4] does not count it */

/* mpcq_config.flags.  MPCQ_FLAG_STATIC_GP: the GP in the model is a static one (use_gp = 1, gpe.type == "GP",
 * src/quad_opt.py:228-236 with src/gp/GP.py:136-175): basis = its training inputs, theta = (L, sigma_f,
 * sqrt(noise + 1e-7)), the training responses are loaded once with mpcq_set_params and the fused step does NOT
 * run the recursive update (mean and covariance stay as they are). */
#define MPCQ_FLAG_STATIC_GP 1

/* MPCQ_PRECISION_F64 (default): the reference's own arithmetic; <= 1e-7 relative control deviation from the fp64 oracle.  (The interior
 * point of a fallback solve iterates in float where the shape allows, N <= 32: it only has to name a working set -- the active-set
 * method behind it, which produces the answer, and everything else are double.)
 * MPCQ_PRECISION_F32: mixed precision (round 5).  Storage and bulk arithmetic in float -- stage records (sensitivities, gaps, cost
 * gradients), Riccati factorisation on the matrix cores, gains, sweeps, RGP state --, the accuracy of double where cond(H) ~ 2e6
 * demands it: the iterate, the measurement and every difference that defines the QP are formed in double (as in F64), the shooting
 * integrates in double and rounds its RECORDS to float once, and the QP solution is kept in double and refined against the residual
 * of the QP evaluated in double on those records, the float factorisation solving for the corrections (iterative refinement).
 * Holds the north_star budget on every solve it reports with status 0 -- warm, cold start, interior-point fallback, saturated inputs:
 * <= 1e-4 relative control deviation from the fp64 oracle, teacher-forced (tests/test_gpu_parity.py; observed <= 2.4e-5, median
 * 2e-8 .. 4e-7).  Status 0 is what every solve of the tests reports and all but two of 7 M audited solves of the bench workload (quadrotors
 * that are lost: flagged / MPCQ_SOLVE_NAN); a solve the float factorisation cannot refine says so (see MPCQ_SOLVE_LOW_ACCURACY). */
#define MPCQ_PRECISION_F64 0
#define MPCQ_PRECISION_F32 1

/* Tuning of the box-QP solve (HPIPM's options in the reference's generated solver have no equivalent here: the
 * algorithm differs, the optimum does not -- the QP is strictly convex).  Every field: 0 = the default for the
 * precision; validated by mpcq_create (MPCQ_ERR_INVALID outside the stated range).  The defaults were measured on two
 * workloads; results do not depend on them beyond rounding.  With MPCQ_TUNING=1 in the
 * environment, MPCQ_WARM_MAX, MPCQ_WARM_RETRY, MPCQ_FLIP_MAX, MPCQ_ABORT_PINS, MPCQ_ABORT_WRONG, MPCQ_POLISH_MAX,
 * MPCQ_PIN_RATIO, MPCQ_IPM_MU0, MPCQ_IPM_MARGIN, MPCQ_IPM_TOL, MPCQ_STAGE_MEM=lds|global|compact, MPCQ_GENERIC=1, MPCQ_BLOCK_ORDER,
 * MPCQ_SPLIT_PLANT=0|1 (the plant update between two lockstep periods as its own launch), MPCQ_GROUPS, MPCQ_KEV_STRIDE, MPCQ_VERBOSE=1 override
 * the corresponding field (measurement scripts only; without MPCQ_TUNING=1 the environment is not consulted). */
typedef struct mpcq_tuning {
  int32_t warm_max;     /* passes of the warm active-set attempt, 1..64 (default 12; 6 in fp64 before round 4) */
  int32_t warm_retry;   /* ... in the period after a fallback solve, 1..64 (default 1) */
  int32_t flip_max;     /* changed bound states in a fallback solve above which the next warm attempt is skipped, 1..512; -1: never (default 2) */
  int32_t abort_pins;   /* warm attempt given up when its first pass pins this many inputs, 1..512; -1: never (default 10, N/2 for N > 20) */
  int32_t abort_wrong;  /* ... or a multiplier check finds this many wrong signs, 1..512; -1: never (default 9, 9N/20 for N > 20) */
  int32_t polish_max;   /* active-set passes behind the interior point, 1..64; -1: none, interior point to qp_tol -- MPCQ_PRECISION_F64 only,
                           refused with MPCQ_PRECISION_F32, whose answer comes from these passes (default 16 f64 / 12 f32) */
  int32_t stage_mem;    /* layout of the per-instance working set: 0 automatic, 1 all LDS, 2 per-stage records in global memory (L2),
                           3 compact (since 0.4: Riccati gains in global memory as well, <= 256 registers: more instances per CU) */
  int32_t generic_kernel; /* 1: the any-shape kernel instance even where a shape-specialised one exists */
  double pin_ratio;     /* interior point -> working set: pinned where multiplier > pin_ratio x slack, (0, 1e3] (default 0.2) */
  double ipm_mu0;       /* complementarity of the interior start in units of the gradient scale, [1e-12, 1] (default 1e-4) */
  double ipm_margin;    /* interior start: distance from the bounds in units of their width, (0, 0.5) (default 0.1) */
  double ipm_tol;       /* interior point -> active-set hand-over tolerance, [qp_tol, 1e-1] (default 1e-6 f64 / 1e-5 f32; f32: not below 1e-5).
                         * fp64 with N <= 32: the float interior point in front hands over at a complementarity of 3e-7 (compile-time), this one
                         * is the tolerance of the double interior point that follows a float one that broke down */
  /* ---- since 0.4 */
  int32_t block_order;  /* launch order of a lockstep period: 0 automatic (quadrotors predicted expensive first when the batch exceeds
                           what the device holds at once), 1 never (workgroup p = quadrotor p), 2 always.  Results do not depend on it. */
  /* ---- since 0.6 (0.4 / 0.5: a reserved field that had to be 0 = automatic) */
  int32_t groups;       /* mpcq_sim_steps: the batch as this many contiguous groups, each advancing in lockstep on a HIP stream of its own,
                           1..16; 0 automatic: 1 for a batch that is resident on the device as a whole, 2 for a larger one (the tail of one
                           group's launch -- the device draining while the last workgroups finish -- is filled by the other group's next
                           launch).  A call still ends with EVERY quadrotor K periods on and quadrotors are independent: results do not
                           depend on it.  mpcq_step / mpcq_step_device_async (one period per call) are always one launch over the batch.
                           More than four groups oversubscribe the hardware queues of the device and are slower. */
} mpcq_tuning;

/* Engine configuration.  Replaces the constructor arguments of quad_optimizer
 * (quad, t_horizon, n_nodes, gpe; src/quad_opt.py:36) and the constants it bakes into the
 * generated solver (weights src/quad_opt.py:122-130, bounds :142-144, quad constants
 * src/quad.py:385-417, RGP basis/theta src/gp/RGP.py:126-157). */
typedef struct mpcq_config {
  int32_t batch;      /* B: number of independent quadrotors in this engine (this rank's shard) */
  int32_t N;          /* n_nodes: shooting intervals */
  int32_t nb;         /* RGP basis points per axis (0: nominal model, use_gp=0) */
  int32_t skip;       /* control_freq_factor = int(optimization_dt / 0.01), src/mpc_controller_node.py:222 */
  double T;           /* t_horizon [s] */
  double dt_pred;     /* step of the nominal prediction: ODOMETRY_DT 0.01 (node) or T/N (python sim) */
  double mass, J[3], max_thrust, x_f[4], y_f[4], z_l_tau[4], g;
  double rotor_drag[3], aero_drag; /* plant only (src/quad.py:79-89); unused by the controller path */
  double W[17], W_e[13];           /* diagonal LS weights; stage cost is scaled by T/N (acados) */
  double u_lb[4], u_ub[4], u_ref[4];
  double qp_tol;      /* KKT tolerance of the interior point's last resort; 0 = default for the precision (1e-11 f64, 1e-5 f32: smaller values
                         are raised to 1e-5 there, the f32 answer is refined against fp64 residuals behind the interior point) */
  const double* basis;   /* [3*nb] basis vectors X per axis */
  const double* theta;   /* [3*3] per axis: L, sigma_f, sigma_n */
  int32_t device;        /* HIP device ordinal */
  int32_t precision;     /* MPCQ_PRECISION_* : arithmetic type of the device path */
  int32_t qp_max_iter;   /* 0 = default */
  int32_t flags;         /* MPCQ_FLAG_* */
  double finish_radius;  /* EPSILON_TRAJECTORY_FINISHED [m], src/mpc_controller_node.py:118; 0 = default 1.0 */
  /* ---- since 0.3 (callers built against an older header: mpcq_create_sized with THEIR sizeof(mpcq_config)) */
  mpcq_tuning tune;      /* all-zero = defaults */
} mpcq_config;

typedef struct mpcq_engine mpcq_engine;

const char* mpcq_last_error(void);
/* "mpcq <major.minor[.patch]> (gfx950, source <16 hex digits>+<8 hex digits>)": the 16 digits are the hash of the sources and the build
 * recipe the library was built from (csrc/Makefile SRC_ID = bench.kernel_source_sha16()); profiles under profiles/ carry the same hash.
 * The 8 behind them (since 0.6.1) hash the device generators of mpcq_replan / mpcq_replan_nonlinear (csrc/mpcq_replan.hpp, since 0.6.2
 * with csrc/mpcq_replan_nl.hpp and csrc/mpcq_minsnap_nl.hpp), since 0.6.3 the flight recorder (csrc/mpcq_record.hpp), since 0.6.4 the RGP
 * read-out (csrc/mpcq_predict.hpp), since 0.6.5 the device missions (csrc/mpcq_mission.hpp), since 0.6.6 the device circle generator
 * (csrc/mpcq_circle.hpp), since 0.6.7 the flight scoreboard (csrc/mpcq_score.hpp) and, with mpcq_rgp_train / mpcq_record_train, the device
 * trainer (csrc/mpcq_train.hpp with csrc/mpcq_learn_core.hpp, which mpcq_learn.hip shares).  The number stays 0.6.7 with the trainer:
 * tests/test_score.py pins it; the eight digits tell a library with the trainer from one without.  The same holds for the fleet
 * (mpcq_fleet_*, csrc/mpcq_fleet.hpp), which joined the eight digits after the trainer, and for the exploration (mpcq_explore_*,
 * csrc/mpcq_explore.hpp), which joined them after the fleet, and the sensor (mpcq_sensor_*, csrc/mpcq_sensor.hpp) after that. */
const char* mpcq_version(void);

/* ---- lifetime.  quad_optimizer.__init__ (src/quad_opt.py:36-160): builds constants, K_x^-1,
 * allocates device state and zero-initialises the iterate (acados default), mu=0, C=K_x. */
/* Versioned form: cfg_size = the caller's sizeof(mpcq_config).  Fields behind cfg_size take their defaults (0), so a
 * caller built against an older header keeps working; sizes that end before `device` or exceed this library's struct
 * are refused. */
int mpcq_create_sized(const mpcq_config* cfg, uint64_t cfg_size, mpcq_engine** out);
/* mpcq_create(cfg, out): for source callers an inline that passes THIS header's sizeof(mpcq_config); the exported symbol of the
 * same name exists for binaries built against the 0.3 header only and reads the 0.3 layout (the struct has grown since: a library
 * that copied its own sizeof would read behind such a caller's struct). */
#ifdef MPCQ_BUILDING_LIBRARY
int mpcq_create(const mpcq_config* cfg, mpcq_engine** out);
#else
static inline int mpcq_create(const mpcq_config* cfg, mpcq_engine** out) { return mpcq_create_sized(cfg, sizeof(mpcq_config), out); }
#endif
int mpcq_destroy(mpcq_engine* e);
int mpcq_reset(mpcq_engine* e);

/* ---- reference.  Fused path: whole sampled trajectories stay on the device and the kernel
 * performs get_reference_chunk (src/utils/utils.py:897-931) + set_reference_trajectory
 * (src/quad_opt.py:295-317) itself.  traj [B, Tmax, 13], len [B] (rows valid per instance);
 * resets the trajectory cursor idx_traj to 0 (src/mpc_controller_node.py:517-552). */
int mpcq_set_trajectories(mpcq_engine* e, const double* traj, const int32_t* len, int32_t Tmax);
/* Explicit path: acados .set(j,'yref',·) for j<N and .set(N,'yref',·)  (src/quad_opt.py:311,315).
 * yref [B, N, 17], yrefN [B, 13]. */
int mpcq_set_reference(mpcq_engine* e, const double* yref, const double* yrefN);
/* acados .set(ii,'p',rgp_params) on every stage (src/quad_opt.py:402-404). mu [B, 3*nb] */
int mpcq_set_params(mpcq_engine* e, const double* mu);

/* ---- quad_optimizer.run_optimization (src/quad_opt.py:321-350): pin x0, ONE SQP-RTI iteration
 * on the persisted iterate, using the stored reference and parameters.  x0 [B, 13]. */
int mpcq_solve(mpcq_engine* e, const double* x0);
/* .get(stage,·): one strided device-to-host copy of the B rows of that stage per call */
int mpcq_get_x(mpcq_engine* e, int32_t stage, double* out);      /* .get(stage,'x') -> [B,13] */
int mpcq_get_u(mpcq_engine* e, int32_t stage, double* out);      /* .get(stage,'u') -> [B,4]  */
int mpcq_get_cost(mpcq_engine* e, double* out);                  /* .get_cost()     -> [B]    */
int mpcq_get_status(mpcq_engine* e, int32_t* out);               /* solve() status  -> [B]    */
/* -> [B]: decimal fields of the last solve.  qp_iter % 1000: Riccati factorisations (active-set passes + interior-point
 * iterations); (qp_iter / 1000) % 10 != 0: the warm active-set attempt was given up or skipped, the solve went through
 * the interior point ("fallback solve"); (qp_iter / 10000) % 10 != 0: that solve also moved more than flip_max inputs
 * on/off their bounds (the next solve skips the warm attempt); qp_iter / 100000: why the warm attempt ended
 * (MPCQ_WARM_*), 0 when it succeeded or there was none (cold start). */
int mpcq_get_qp_iter(mpcq_engine* e, int32_t* out);
/* What the last solve of every quadrotor executed, out [B] (read as unsigned): Riccati factorisations (bits 0..14; resumed ones count
 * as whole) | matrix-vector sweeps over the horizon (bits 16..26, saturating) | since 0.6, bits 27..31: how many of the interior-point
 * iterations ran in float (fp64 instances whose interior point iterates in float, N <= 32 on a shape-specialised instance: all of a
 * fallback solve's, unless bit 15 is set; 0 everywhere else -- a latency model prices exactly these with the float chains).  Bit 15 (fp64
 * instances): the float interior point of a fallback solve broke down and the double one ran from the start (a diagnostic: the answer
 * comes from the double active-set method either way).  The dependent chains of these are what a lockstep launch lasts
 * (bench.py `latency_roofline`).  acados reports sqp_iter / qp_iter through get_stats (src/quad_opt.py:337 reads time_tot only). */
int mpcq_get_qp_work(mpcq_engine* e, int32_t* out);
#define MPCQ_WARM_BUDGET 1    /* pass budget (warm_max / warm_retry) exhausted */
#define MPCQ_WARM_PINS 2      /* first pass pinned >= abort_pins inputs */
#define MPCQ_WARM_WRONG 3     /* a multiplier check found >= abort_wrong wrong signs */
#define MPCQ_WARM_BOUNCE 4    /* a bulk release bounced back with most inputs saturated */
#define MPCQ_WARM_NUMERIC 5   /* a stage Hessian was not positive definite / not a number */
#define MPCQ_WARM_SKIPPED 6   /* skipped: the previous solve carried the flip mark */
/* .get_stats('time_tot'): device time of the last solve/step launch in seconds (whole batch) */
int mpcq_get_stats(mpcq_engine* e, double* time_tot);

/* ---- quad_optimizer.discrete_dynamics on the nominal model (src/quad_opt.py:353-377,
 * src/mpc_controller_node.py:298).  x [B,13], u [B,4] -> out [B,13] */
int mpcq_predict_nominal(mpcq_engine* e, const double* x, const double* u, double dt, double* out);

/* ---- quad_optimizer.regress_and_update_RGP_model (src/quad_opt.py:380-406): 3 scalar RGP
 * Kalman updates per instance and the new means become the stage parameters.
 * v_body [B,3], a_drag [B,3]. */
int mpcq_rgp_regress(mpcq_engine* e, const double* v_body, const double* a_drag);
int mpcq_get_rgp(mpcq_engine* e, double* mu /*[B,3,nb] or NULL*/, double* C /*[B,3,nb,nb] or NULL*/);

/* ---- fused control step = the loop body src/mpc_controller_node.py:278-318
 * (src/execute_trajectory.py:202-258): chunk -> yref -> solve -> w=U[0] -> nominal prediction ->
 * idx_traj++ -> compute_a_drag -> RGP regress -> params.  x_meas [B,13] -> w_out [B,4];
 * x_pred_out [B,13] may be NULL. */
int mpcq_step(mpcq_engine* e, const double* x_meas, double* w_out, double* x_pred_out);
/* Same with device-resident buffers: d_x_meas [B,13] and d_w_out [B,4] (NULL: engine-internal) are
 * float64 device pointers in EVERY precision (the measurement and the iterate are always double; the
 * precision only selects the arithmetic of the QP).  No host traffic, no synchronisation; ordered on
 * the engine's stream. */
int mpcq_step_device_async(mpcq_engine* e, const double* d_x_meas, double* d_w_out);
int mpcq_synchronize(mpcq_engine* e);
void* mpcq_stream(mpcq_engine* e);   /* hipStream_t the engine launches on */

/* ---- command mapping of publish_control_gazebo (src/mpc_controller_node.py:600-612) for the last
 * step / solve: rotor_thrusts [B,4] = w * max_thrust / mass, collective_thrust [B] = sum(w) * max_thrust
 * / mass, bodyrates [B,3] = x_opt[1, 10:13] (src/mpc_controller_node.py:292).  Any pointer may be NULL. */
int mpcq_get_command(mpcq_engine* e, double* rotor_thrusts, double* collective_thrust, double* bodyrates);
/* ---- trajectory finished (src/mpc_controller_node.py:374): per instance 1 once a fused step found
 * idx_traj + 1 == len(trajectory) (after its idx_traj += 1) with the quadrotor closer than
 * finish_radius to the first row of that step's reference chunk; sticky until mpcq_set_trajectories
 * or mpcq_reset.  out [B]. */
int mpcq_get_finished(mpcq_engine* e, int32_t* out);
/* get_reference_chunk (src/utils/utils.py:897-931) at the current cursor, evaluated on the device
 * with the row selection of the fused step.  out [B, N, 13]. */
int mpcq_get_reference_chunk(mpcq_engine* e, double* out);

/* ---- closed-loop harness on the device: Quadrotor3D.update with drag
 * (src/quad.py:166-190,234-277,329-357) applied n_sub times with step sim_dt to the engine's
 * internal plant state, driven by the last w.  mpcq_sim_reset sets the plant state [B,13];
 * mpcq_sim_steps runs K closed-loop iterations {step(x) -> plant} without host round trips. */
int mpcq_sim_reset(mpcq_engine* e, const double* x0);
int mpcq_sim_steps(mpcq_engine* e, int32_t K, int32_t n_sub, double sim_dt);
/* The same K closed-loop iterations as ONE launch in which every instance runs through its K control periods
 * without waiting for the others (instances are independent; src/execute_trajectory.py:196-279 is a loop over ONE
 * quadrotor).  Same arithmetic, same results as mpcq_sim_steps; the per-period outputs readable afterwards
 * (mpcq_get_*, mpcq_sim_get_state) are those of the last period (per-period logs: the flight recorder with mpcq_sim_steps;
 * MPCQ_ERR_STATE while a recording is active, see mpcq_record_start). */
int mpcq_sim_run(mpcq_engine* e, int32_t K, int32_t n_sub, double sim_dt);
/* The reference's plant loop between two solves (src/execute_trajectory.py:232-243):
 * `while control_time < optimization_dt: quad.update(w, simulation_dt); control_time += simulation_dt`.
 * mpcq_plant_substeps reproduces its iteration count with the same double accumulation (20 / 11 / 4
 * substeps for control_dt = 0.1 / 0.05 / 0.02 at sim_dt = 5e-3); negative on bad arguments.
 * mpcq_sim_plant_period advances the plant state by that loop with control w [B,4] (NULL: the last
 * control of the engine); mpcq_sim_control_periods = K x {fused step -> that loop}. */
int mpcq_plant_substeps(double control_dt, double sim_dt);
int mpcq_sim_plant_period(mpcq_engine* e, const double* w, double control_dt, double sim_dt, int32_t* n_sub /*out, may be NULL*/);
int mpcq_sim_control_periods(mpcq_engine* e, int32_t K, double control_dt, double sim_dt, int32_t* n_sub /*out, may be NULL*/);
int mpcq_sim_get_state(mpcq_engine* e, double* x /*[B,13]*/, double* w /*[B,4] or NULL*/);
/* HIP-event time of the step-kernel launches of the last mpcq_sim_steps / mpcq_sim_run call (events recorded on
 * the engine's stream around every 4th launch, MPCQ_KEV_STRIDE=1 for every launch): total seconds of the timed
 * launches and their number (mpcq_tuning.groups > 1: the launches of group 0, see mpcq_get_groups). */
int mpcq_get_kernel_time(mpcq_engine* e, double* seconds, int32_t* launches);
int mpcq_get_kernel_time_minmax(mpcq_engine* e, double* fastest_s, double* slowest_s);   /* of the same timed launches */
/* diagnostic build only (libmpcq_prof.so, -DMPCQ_PROFILE): per-instance shader-cycle totals per phase of
 * the last step, out [B][16]; MPCQ_ERR_STATE in the product build. */
int mpcq_debug_profile(mpcq_engine* e, unsigned long long* out);
/* The launch order of the last lockstep period, out [B]: workgroup p ran quadrotor out[p] (mpcq_tuning.block_order; the
 * identity when no order is in use).  The reference solves one quadrotor per process (src/quad_opt.py:321-350) and has no
 * counterpart; results do not depend on the order. */
int mpcq_get_block_order(mpcq_engine* e, int32_t* out);
/* Since 0.6.  The number of groups mpcq_sim_steps runs this engine's batch in (mpcq_tuning.groups resolved: 1 = one launch per period
 * over the whole batch).  With more than one group the launches mpcq_get_kernel_time reports are group 0's -- a launch over B / groups
 * quadrotors that shares the device with the other groups' launches: per-period figures come from the caller's clock around the call.
 * No counterpart in the reference (one quadrotor per process, src/quad_opt.py:321-350). */
int mpcq_get_groups(mpcq_engine* e, int32_t* out);

/* ---- tracking statistic (src/Visualiser.py:787-789,809-811,918), summed over this engine's
 * instances since the last reset: out[0]=sum |e_pos|^2, out[1]=sum |e_vel|^2, out[2]=steps,
 * out[3]=max |e_pos|^2, out[4]=instances with status != 0 in the last step. */
int mpcq_get_tracking_stats(mpcq_engine* e, double out[5]);

/* ---- multi-GPU: one engine per rank; the only collective is the reduction of the statistics
 * vector (RCCL over xGMI).  The host exchanges the 128-byte unique id however it likes. */
int mpcq_comm_unique_id(void* id128);
int mpcq_comm_init(mpcq_engine* e, int32_t rank, int32_t nranks, const void* id128);
/* A second engine of the same process and device reduces over the communicator `owner` initialised (since 0.5): one rank = one
 * communicator however many engines it runs (bench.py: the configs[3] swarm next to the configs[1] headline).  `e` borrows the
 * handle, `owner` has to outlive it (or `e` must not reduce any more); calls on the two engines must not overlap in time.
 * The RCCL library is dlopen'ed by name (librccl.so, then /opt/rocm/lib/librccl.so); MPCQ_RCCL_LIB in the environment names another file. */
int mpcq_comm_share(mpcq_engine* e, mpcq_engine* owner);
/* sum (out[0..2], out[4]) / max (out[3]) over ranks; every rank receives the result */
int mpcq_allreduce_tracking_stats(mpcq_engine* e, double out[5]);

/* ---- state dump / restore (teacher-forced parity tests, checkpoint/resume).  Any pointer may
 * be NULL.  X [B,N+1,13], U [B,N,4], mu [B,3,nb], C [B,3,nb,nb], x_pred_prev [B,13],
 * has_prev [B], idx [B]. */
int mpcq_get_state(mpcq_engine* e, double* X, double* U, double* mu, double* C, double* x_pred_prev,
                   int32_t* has_prev, int32_t* idx);
int mpcq_set_state(mpcq_engine* e, const double* X, const double* U, const double* mu, const double* C,
                   const double* x_pred_prev, const int32_t* has_prev, const int32_t* idx);

/* The rest of the resumable state: warm-start flag / pass count of the last solve qp_iter [B], the
 * tracking accumulators stats [B,4] (sum |e_pos|^2, sum |e_vel|^2, steps, max |e_pos|^2) and the
 * finished flags [B].  With mpcq_get_state + mpcq_sim_get_state a restored engine continues bit for bit. */
int mpcq_get_solver_state(mpcq_engine* e, int32_t* qp_iter, double* stats, int32_t* finished);
int mpcq_set_solver_state(mpcq_engine* e, const int32_t* qp_iter, const double* stats, const int32_t* finished);

/* ---- continuous operation (since 0.6.1): a finished flight is followed by the next one, planned from where the quadrotor stands
 * (src/mpc_controller_node.py:372-399 -> request_trajectory :430-453 -> trajectory_received_cb :511-552), for the selected quadrotors
 * only while the others keep flying.  Per-quadrotor result codes of mpcq_replan, out[b]: */
#define MPCQ_REPLAN_DONE 0          /* new flight installed */
#define MPCQ_REPLAN_SKIPPED 1       /* not selected */
#define MPCQ_REPLAN_BAD_INPUT (-1)  /* non-finite start or waypoint */
#define MPCQ_REPLAN_SINGULAR (-2)   /* as mpcq_traj.h -2 (reserved: like mpcq_minsnap_generate_order, the bisection counts a singular
                                       solve as a limit violation, so such a flight ends in MPCQ_REPLAN_LIMITS) */
#define MPCQ_REPLAN_LIMITS (-3)     /* as mpcq_traj.h -3: the limits cannot be met */
#define MPCQ_REPLAN_TOO_LONG (-4)   /* the sampled flight has more rows than the Tmax of mpcq_set_trajectories */
/* Minimum-snap flights planned and sampled on the device, one wavefront per selected quadrotor: for the vertices
 * [start_b, wp[b,0], ..., wp[b,n_wp-1]] exactly the host generator's result, mpcq_minsnap_generate_order(.., v_max, a_max,
 * derivative_to_optimize, ..) sampled like mpcq_minsnap_sample(.., dt) (positions / velocities may differ by one quantum of the
 * 6-decimal rounding).  Selected: mask[b] != 0, or with mask == NULL the quadrotors whose finished flag is set on the device.
 * start [B,3]; NULL: the position of the on-device plant (mpcq_sim_get_state; MPCQ_ERR_STATE without an earlier mpcq_sim_reset).
 * On MPCQ_REPLAN_DONE the slot gets the new rows (padded with the last one up to Tmax), len[b] = the row count, the cursor goes to
 * 0 and the finished flag to 0; nothing else of the quadrotor changes (iterate, RGP, x_pred_prev, has_prev, QP status, tracking
 * accumulators).  A negative code leaves trajectory, cursor and finished flag as they were.  Waypoints of unselected quadrotors are
 * not read for validity.  MPCQ_ERR_INVALID: n_wp outside 1..7, v_max / a_max / dt not > 0, derivative_to_optimize outside 2..4,
 * wp NULL; MPCQ_ERR_STATE before mpcq_set_trajectories.  out [B] may be NULL. */
int mpcq_replan(mpcq_engine* e, const double* start /*[B,3] or NULL*/, const double* wp /*[B,n_wp,3]*/, int32_t n_wp,
                double v_max, double a_max, int32_t derivative_to_optimize, double dt,
                const int32_t* mask /*[B] or NULL*/, int32_t* out /*[B] or NULL*/);
/* Since 0.6.2.  mpcq_replan with the reference generator's nonlinear stage: for each selected quadrotor exactly the host library's
 * mpcq_minsnap_nonlinear(.., v_max, a_max, derivative_to_optimize, opts, ..) -- segment times and free vertex derivatives optimised by
 * Subplex from the linear stage, soft speed / acceleration limits -- sampled like mpcq_minsnap_sample(.., dt).  Selection, start, result
 * codes and install as mpcq_replan (MPCQ_REPLAN_SINGULAR: the linear stage's system is singular; MPCQ_REPLAN_LIMITS: the linear stage
 * lasts longer than 300 s, which mpcq_minsnap_nonlinear refuses too: segment times are bounded above by 10 x their start).  Soft limits: a flight may exceed
 * v_max / a_max and is installed anyway; info reports its peaks.  opts NULL: the defaults.  Optional outputs (NaN rows for quadrotors
 * without a result): info [B,6] = f at the start, f at the end, evaluations, total duration, peak speed, peak acceleration;
 * pieces [B,n_wp,33]; d_free [B,n_wp-1,3,3].  MPCQ_ERR_INVALID as mpcq_replan, plus options outside the rules of include/mpcq_nl_options.h (time_penalty must be > 0). */
int mpcq_replan_nonlinear(mpcq_engine* e, const double* start /*[B,3] or NULL*/, const double* wp /*[B,n_wp,3]*/, int32_t n_wp,
                          double v_max, double a_max, int32_t derivative_to_optimize, double dt,
                          const int32_t* mask /*[B] or NULL*/, int32_t* out /*[B] or NULL*/, const mpcq_minsnap_nl_options* opts /*or NULL*/,
                          double* info /*[B,6] or NULL*/, double* pieces /*[B,n_wp,33] or NULL*/, double* d_free /*[B,n_wp-1,3,3] or NULL*/);
/* Since 0.6.6.  The reference's 'circle' request (src/mpc_controller_node.py:430-453 -> sample_circle_trajectory_acc_dec(radius, v_max,
 * dt, start_point)) generated on the device, one wavefront per selected quadrotor: the closed-form circle flights of the reference's
 * TrajectoryGenerator (src/trajectory_generation/TrajectoryGenerator.py:41-131), a circle of radius[b] that starts at start_b and is
 * flown in the x-y plane at the start's height, q = [1,0,0,0], body rates 0, positions / velocities rounded to 6 decimals. */
#define MPCQ_CIRCLE_ACC_DEC 0       /* one round: angular speed up to v_max / radius at half time, then down again (the node's request) */
#define MPCQ_CIRCLE_CONSTANT 1      /* one round at v_max */
#define MPCQ_CIRCLE_ACCELERATING 2  /* t_max seconds, angular speed 0 -> v_max / radius -> 0 on a raised cosine */
/* The row count is that of the reference (ceil(stop / dt), `stop` formed by its expression in double) and the running sums of angular
 * speed and angle are accumulated in row order, so a flight differs from the host's trajectories.circle_trajectory by the device's
 * sin / cos only: at most one quantum of the 6-decimal rounding, in rare entries.  radius [B], v_max [B]: per quadrotor; t_max is read for
 * MPCQ_CIRCLE_ACCELERATING only.  Selection (mask / finished flags), start (NULL: the plant position), install and `out` as mpcq_replan.
 * Codes: MPCQ_REPLAN_BAD_INPUT: start, radius or v_max not finite, or radius / v_max not > 0; MPCQ_REPLAN_TOO_LONG: more rows than Tmax;
 * a negative code leaves trajectory, cursor and finished flag as they were.  MPCQ_ERR_INVALID: radius or v_max NULL, unknown kind, dt
 * (MPCQ_CIRCLE_ACCELERATING: or t_max) not finite and > 0; MPCQ_ERR_STATE as mpcq_replan. */
int mpcq_replan_circle(mpcq_engine* e, const double* start /*[B,3] or NULL*/, const double* radius /*[B]*/, const double* v_max /*[B]*/,
                       int32_t kind, double dt, double t_max /*ACCELERATING only*/, const int32_t* mask /*[B] or NULL*/,
                       int32_t* out /*[B] or NULL*/);
/* The same slot install for host-made rows (the reference's 'line' request, or any other flight): quadrotors idx[0..count), rows
 * traj [count, Tmax, 13] of which the first len[j] are used; 1 <= len <= Tmax, indices in range and unique. */
int mpcq_replace_trajectories(mpcq_engine* e, const int32_t* idx /*[count]*/, int32_t count,
                              const double* traj /*[count,Tmax,13]*/, const int32_t* len /*[count]*/);
/* The trajectory buffer and lengths as they are now.  A checkpoint after replans restores with mpcq_set_trajectories(traj, len),
 * then mpcq_set_state(idx = ...) and mpcq_set_solver_state(finished = ...). */
int mpcq_get_trajectories(mpcq_engine* e, double* traj /*[B,Tmax,13] or NULL*/, int32_t* len /*[B] or NULL*/);

/* ---- device missions (since 0.6.5): the node requests the next flight in the callback that sees the finish
 * (src/mpc_controller_node.py:372-399); here a queue of upcoming flights per quadrotor lives on the device and a launch behind every
 * period installs the next one for whoever just finished, with no host round trip.  A period is what the flight recorder counts: one
 * mpcq_step / mpcq_step_device_async call, one iteration of mpcq_sim_steps / mpcq_sim_control_periods; mpcq_solve is not a period.
 * Per quadrotor, behind every period: if its finished flag is set and leg[b] < L, a flight is planned through [start, wp[b, leg[b]]] --
 * exactly what mpcq_replan (nonlinear = 0) or mpcq_replan_nonlinear (nonlinear = 1, options opts) would plan -- and installed as they
 * install it (rows, padding, length, cursor 0, flag 0).  start is the plant position behind that period's plant update
 * (mpcq_sim_steps / mpcq_sim_control_periods) or the period's measurement x_meas[b, 0:3] (mpcq_step, mpcq_step_device_async): the start
 * points a host loop `sim_steps(1); replan(mask = finished & (leg < L))` passes, and the results are bit for bit that loop's.  The leg
 * is consumed whatever the MPCQ_REPLAN_* code: a negative code leaves trajectory, cursor and flag as they were and the next period
 * tries the next leg.  A quadrotor whose queue is exhausted (leg[b] == L) holds its last reference row, as without a mission.
 * On the stream of a period the order is: recorder snapshot -> black-box snapshot -> ordering launch -> step -> recorder row ->
 * black box -> score -> exploration -> plant -> mission (each only while its feature is on); a recorded
 * row of the finishing period shows finished = 1 and the old cursor, the next row cursor 0 of the new flight.  While a mission is
 * active every plant update of mpcq_sim_steps is a launch of its own (same arithmetic, same results as the fused form).
 * mpcq_sim_run (one persistent launch) flies no mission: MPCQ_ERR_STATE while one is active.  Host calls of mpcq_replan* and
 * mpcq_replace_trajectories stay legal and consume no legs.  With no mission set every launch sequence and result is what it was.
 *
 * mpcq_mission_set uploads the queue wp [B,L,n_wp,3] and the leg counters leg0 [B] (NULL: 0; values 0..L -- a checkpoint restores with
 * the leg of mpcq_mission_get) and resets the log and the period count; calling it again replaces the queue.  MPCQ_ERR_INVALID: wp NULL,
 * n_wp outside 1..7, L < 1, v_max / a_max / dt not finite and > 0, derivative_to_optimize outside 2..4, nonlinear not 0 / 1, options
 * outside the rules of include/mpcq_nl_options.h, leg0 outside 0..L.  MPCQ_ERR_STATE before mpcq_set_trajectories. */
int mpcq_mission_set(mpcq_engine* e, const double* wp /*[B,L,n_wp,3]*/, int32_t L, int32_t n_wp, double v_max, double a_max,
                     int32_t derivative_to_optimize, double dt, int32_t nonlinear, const mpcq_minsnap_nl_options* opts /*or NULL*/,
                     const int32_t* leg0 /*[B] or NULL*/);
/* Since 0.6.6: a kind and limits per leg.  The reference sends v_max / a_max with every request and one of its request types is a circle;
 * here quadrotor b flies leg l as legs[b, l] says, so a sweep over the limits is one batch.  mpcq_mission_set is the special case in
 * which every leg is MPCQ_LEG_WAYPOINTS with that call's v_max / a_max. */
#define MPCQ_LEG_WAYPOINTS 0   /* min-snap through wp[b, leg] (linear or nonlinear as the mission says) */
#define MPCQ_LEG_CIRCLE    1   /* MPCQ_CIRCLE_ACC_DEC of `radius` at `v_max` from where the quadrotor stands */
typedef struct mpcq_leg { int32_t kind, reserved; double v_max, a_max, radius; } mpcq_leg;
/* legs [B,L] is uploaded once; everything else (claiming, leg consumption, the log, mpcq_mission_get / mpcq_mission_stop, the start
 * point, dt) is mpcq_mission_set's.  A waypoint leg is planned through wp[b, leg] with its own v_max / a_max (radius is not read), a
 * circle leg is what mpcq_replan_circle(MPCQ_CIRCLE_ACC_DEC, radius, v_max, dt) installs (a_max is checked, not used; wp[b, leg] is not
 * read); info is NaN after a circle leg.  wp may be NULL if no leg is a waypoint leg (n_wp is not read then).  MPCQ_ERR_INVALID: legs
 * NULL, an unknown kind, reserved != 0, a waypoint leg with wp NULL, v_max / a_max of any leg or the radius of a circle leg not finite
 * and > 0, and the rules of mpcq_mission_set for L, n_wp (with wp), dt, derivative_to_optimize, nonlinear, opts and leg0. */
int mpcq_mission_set_legs(mpcq_engine* e, const mpcq_leg* legs /*[B,L]*/, const double* wp /*[B,L,n_wp,3]; NULL iff no waypoint leg*/,
                          int32_t L, int32_t n_wp, int32_t derivative_to_optimize, double dt, int32_t nonlinear,
                          const mpcq_minsnap_nl_options* opts /*or NULL*/, const int32_t* leg0 /*[B] or NULL*/);
/* The mission's state, behind everything the engine has enqueued; every pointer may be NULL.  leg [B]: legs consumed so far;
 * installed [B]: flights installed; last_code [B]: code of the last consumed leg (MPCQ_REPLAN_SKIPPED: none yet); leg_code [B,L]: code
 * of every leg (MPCQ_REPLAN_SKIPPED: not consumed); leg_period [B,L]: the period number since mpcq_mission_set in which the leg was
 * consumed, -1 if it has not been; info [B,6] (nonlinear: the info row of mpcq_replan_nonlinear for the last installed flight, NaN
 * before the first; linear: NaN).  MPCQ_ERR_STATE: no mission set. */
int mpcq_mission_get(mpcq_engine* e, int32_t* leg /*[B]*/, int32_t* installed /*[B]*/, int32_t* last_code /*[B]*/,
                     int32_t* leg_code /*[B,L]*/, int32_t* leg_period /*[B,L]*/, double* info /*[B,6]*/);
/* Mission off, the queue freed: period launches are exactly what they are without one.  MPCQ_ERR_STATE: no mission set. */
int mpcq_mission_stop(mpcq_engine* e);

/* ---- flight recorder (since 0.6.3): per-period logs of a swarm that flies on the device (the reference appends one row per control
 * step, src/mpc_controller_node.py:353-364, src/execute_trajectory.py:269-275).  A period is one fused step of every quadrotor: one
 * mpcq_step / mpcq_step_device_async call, one iteration of mpcq_sim_steps / mpcq_sim_control_periods.  Periods count from
 * mpcq_record_start; period k is recorded when k % every == 0, one row per selected quadrotor, written on the device by a launch behind
 * the step launch (and, with MPCQ_RECORD_DRAG, a launch in front of it); the host reads the buffers once.  Recording changes no
 * result of the engine.  mpcq_solve is not a period.  mpcq_reset, mpcq_set_state, mpcq_set_trajectories and the replan calls are
 * allowed during a recording and show in later rows.  mpcq_sim_run (one persistent launch) does not record: MPCQ_ERR_STATE while a
 * recording is active.  Every value is stored as float64 (MPCQ_PRECISION_F32: mu and C converted as mpcq_get_rgp converts them).
 * Fields (bit mask) and the width of one row: */
#define MPCQ_RECORD_X_ODOM   1    /* [13] the measurement the step solved from (plant state at the period start / the caller's x_meas) */
#define MPCQ_RECORD_X_REF    2    /* [13] row 0 of the reference chunk the step used (the node's x_ref; the row of the tracking statistic) */
#define MPCQ_RECORD_W        4    /* [4]  the control of the step */
#define MPCQ_RECORD_X_PRED   8    /* [13] the nominal prediction of the step */
#define MPCQ_RECORD_COST    16    /* [1]  cost of the step */
#define MPCQ_RECORD_DRAG    32    /* [6]  v_body(3), a_drag(3): compute_a_drag of the measurement against the x_pred_prev the step started from */
#define MPCQ_RECORD_RGP_MU  64    /* [3*nb] RGP mean after the step (nb > 0 only) */
#define MPCQ_RECORD_RGP_C  128    /* [3*nb*nb] RGP covariance after the step (nb > 0 only) */
#define MPCQ_RECORD_SOLVER 256    /* [4] int32: status, qp_iter, trajectory cursor the step used, finished flag after the step */
/* Starts a recording of quadrotors quads[0..count) (NULL: all B, count ignored), `capacity` rows per quadrotor.  A full buffer does not
 * wrap: later recorded periods count as dropped (mpcq_record_clear empties it).  Memory: capacity x count x (sum of the widths) x 8 bytes.
 * MPCQ_ERR_INVALID: count <= 0 with quads, an index out of range or twice, fields 0 or unknown bits, every < 1, capacity < 1, an RGP
 * field with nb = 0.  MPCQ_ERR_STATE: a recording is active.  MPCQ_ERR_DEVICE: the buffers cannot be allocated. */
int mpcq_record_start(mpcq_engine* e, const int32_t* quads /*[count] or NULL*/, int32_t count, int32_t fields, int32_t every, int32_t capacity);
/* rows recorded, periods dropped (buffer full), periods counted since mpcq_record_start.  Any pointer may be NULL. */
int mpcq_record_info(mpcq_engine* e, int32_t* rows, int64_t* dropped, int64_t* periods);
/* One recorded double field (a single MPCQ_RECORD_* bit other than MPCQ_RECORD_SOLVER, else MPCQ_ERR_INVALID), out [count, rows, width]:
 * quadrotors in the caller's order of mpcq_record_start, rows in time order. */
int mpcq_record_get(mpcq_engine* e, int32_t field, double* out);
int mpcq_record_get_solver(mpcq_engine* e, int32_t* out /*[count, rows, 4]*/);
int mpcq_record_get_periods(mpcq_engine* e, int64_t* out /*[rows]: the period number of each row*/);
/* rows = 0 and dropped = 0; the selection, the fields and the period count stay */
int mpcq_record_clear(mpcq_engine* e);
/* frees the buffers; recording off.  get / info / clear / stop without an active recording: MPCQ_ERR_STATE. */
int mpcq_record_stop(mpcq_engine* e);

/* ---- incident recorder: a black box per quadrotor.  In a sweep that flies as one batch some quadrotors get lost, and which ones is not
 * known beforehand.  The scoreboard shows that something went wrong, the flight recorder shows what -- but only for quadrotors chosen
 * before the run, with memory that grows with its length.  A black box watches `count` quadrotors (quads, or all B): each gets a ring of
 * D = pre + 1 + post of the flight recorder's rows, overwritten every period, and a rule of its own that is judged on the device; the
 * ring stops `post` periods after the rule first fires.  Memory: count x D x (sum of the widths) x 8 bytes, whatever the length of the
 * run, and no host round trip.  The fields are the flight recorder's MPCQ_RECORD_* bits, with its widths and its float64 storage.
 *   Periods p = 0, 1, ... count from mpcq_blackbox_start as the flight recorder counts them: one mpcq_step / mpcq_step_device_async
 * call, one iteration of mpcq_sim_steps / mpcq_sim_control_periods; mpcq_solve is not a period.
 *   Per watched quadrotor the device keeps state (0 armed, 1 fired, 2 frozen), fired_period (-1), cause (0), left and first (the first
 * period whose row the ring holds).  In period p, for a quadrotor that is not frozen:
 *  1. Its row of every requested field goes to ring slot p % D: bit for bit the values the flight recorder writes for that period
 *     (MPCQ_RECORD_DRAG against the x_pred_prev the step started from, MPCQ_RECORD_X_REF row 0 of the chunk the step used).
 *  2. The rule is judged on the period's values and gives a cause word c.  Armed and c != 0: fired_period = p, cause = c, state = 1,
 *     left = post.  Already in state 1 before this period: left -= 1.  In state 1 with left == 0: state = 2 (with post = 0, in the
 *     firing period itself).
 * A frozen quadrotor's ring is no longer written: it holds exactly the periods max(first, f - pre) .. f + post of the first incident.
 *   Causes (bits of rule.causes; a cause that is not enabled is never raised; all causes true in the firing period are reported together),
 * with x the measurement the step solved from, ref the MPCQ_RECORD_X_REF row, w the control and cost the cost of the step: */
#define MPCQ_BB_STATUS     1   /* status & rule.status_mask is non-zero */
#define MPCQ_BB_FALLBACK   2   /* the period's solve was a fallback solve: qp_iter / 1000 % 10 != 0 (the scoreboard's `fallbacks`) */
#define MPCQ_BB_NONFINITE  4   /* any entry of x, w or the cost is not finite */
#define MPCQ_BB_ERR_POS    8   /* ((dx*dx + dy*dy) + dz*dz) > err_pos*err_pos, d = x[0:3] - ref[0:3] */
#define MPCQ_BB_SPEED     16   /* ((vx*vx + vy*vy) + vz*vz) > speed*speed, v = x[7:10] */
#define MPCQ_BB_TILT      32   /* 1 - 2*(qx*qx + qy*qy) < tilt_cos (body z against world z), q = x[3:7] */
#define MPCQ_BB_COST      64   /* cost > rule.cost */
/* The sums of squares and the tilt expression are evaluated in the order written, every operation rounded on its own (no fused
 * multiply-add), so a host reproduces them exactly from recorded rows.  A comparison with a NaN operand is false: NaN is what
 * MPCQ_BB_NONFINITE is for.
 *   The black box changes no result: with it on or off every state, output and statistic is bit-identical, and so is every row of a
 * flight recorder or scoreboard running next to it.  It runs together with the recorder, score, mission, exploration and fleet and does
 * not depend on mpcq_tuning.groups; mpcq_reset, mpcq_set_state and the replan calls are legal while it runs.  On the stream of a period
 * the order is: recorder snapshot -> black-box snapshot -> ordering launch -> step -> recorder row -> black box -> score -> exploration
 * -> plant -> mission.  mpcq_sim_run (one persistent launch) keeps no black box: MPCQ_ERR_STATE while one runs.  A black box is per
 * engine (per shard) and not part of a checkpoint, like a recording. */
typedef struct mpcq_blackbox_rule { int32_t causes, status_mask; double err_pos, speed, tilt_cos, cost; } mpcq_blackbox_rule;   /* one per watched quadrotor */
/* Starts a black box for quadrotors quads[0..count) (NULL: all B, count ignored) with rules [count] in the same order.
 * MPCQ_ERR_STATE: a black box runs.  MPCQ_ERR_INVALID, with the engine left as it was: count <= 0 with quads, an index out of range or
 * twice, fields 0 or unknown bits, an RGP field with nb = 0, pre or post negative, D > 65536, rules NULL, and -- mpcq_last_error() names
 * the quadrotor and the field -- unknown cause bits, a NaN threshold of an enabled cause, err_pos or speed < 0.  MPCQ_ERR_DEVICE: the
 * buffers cannot be allocated. */
int mpcq_blackbox_start(mpcq_engine* e, const int32_t* quads /*[count] or NULL*/, int32_t count, int32_t fields, int32_t pre, int32_t post,
                        const mpcq_blackbox_rule* rules /*[count], caller's order*/);
/* The state of every watched quadrotor in the caller's order, behind everything the engine has enqueued; any pointer may be NULL.
 * rows [count]: min(D, periods written since first) -- for a quadrotor that has fired, the rows of its incident so far: the periods
 * max(first, f - pre) .. min(f + post, the last period); fired_row [count]: the index of the firing row in the time-ordered read-out
 * (-1: not fired); periods: periods counted since mpcq_blackbox_start. */
int mpcq_blackbox_info(mpcq_engine* e, int64_t* fired_period, int32_t* cause, int32_t* state, int32_t* rows, int32_t* fired_row /*each [count] or NULL*/,
                       int64_t* periods);
/* The rings of a subset, gathered on the device into time order and left-aligned: which [n] are positions in the selection (the caller's
 * order of mpcq_blackbox_start; NULL: the whole selection, n ignored), out [n, D, width] for one double field (a single MPCQ_RECORD_*
 * bit of the black box other than MPCQ_RECORD_SOLVER).  Row k of item i is period first_row_period + k; rows beyond rows[i] are NaN
 * (-1 for the solver ints and the period numbers).  Only n rings travel to the host.  MPCQ_ERR_INVALID: a field the black box does not
 * keep, a position outside [0, count) or twice. */
int mpcq_blackbox_get(mpcq_engine* e, int32_t field, const int32_t* which /*[n] positions in the selection, or NULL: all*/, int32_t n, double* out /*[n, D, width]*/);
int mpcq_blackbox_get_solver(mpcq_engine* e, const int32_t* which, int32_t n, int32_t* out /*[n, D, 4]*/);
int mpcq_blackbox_get_periods(mpcq_engine* e, const int32_t* which, int32_t n, int64_t* out /*[n, D]*/);
/* The selected quadrotors (mask [count] non-zero, caller's order; NULL: all) back to armed with an empty ring: first = the next period,
 * fired_period = -1, cause = 0.  The others keep what they hold. */
int mpcq_blackbox_rearm(mpcq_engine* e, const int32_t* mask /*[count] or NULL*/);
/* frees the buffers; black box off, period launches are what they are without one.  Every call but mpcq_blackbox_start without a
 * running black box: MPCQ_ERR_STATE. */
int mpcq_blackbox_stop(mpcq_engine* e);

/* ---- flight scoreboard (since 0.6.7): the reference evaluates a run flight by flight -- src/compare_trajectories.py:40-51 plots, per
 * flight, max ||v|| against the mean of the per-step rms_pos of src/Visualiser.py:805-822 and leaves out the last second "because it
 * tries to stop in place".  Here a table score [B, F, 16] of doubles lives on the device and one small launch behind every period folds
 * that period into the row of the flight the quadrotor is flying; the host reads the table once, at the end of a sweep.  A period is
 * what the flight recorder and the missions count: one mpcq_step / mpcq_step_device_async call, one iteration of mpcq_sim_steps /
 * mpcq_sim_control_periods; mpcq_solve is not a period.  On the stream of a period the order is: recorder snapshot -> black-box
 * snapshot -> ordering launch -> step -> recorder row -> black box -> score -> exploration -> plant -> mission, so the score reads what a recorded row shows: the measurement x the step solved
 * from, the cursor i the step used, ref = row 0 of the reference chunk the step used (MPCQ_RECORD_X_REF), status, qp_iter, cost and the
 * finished flag after the step.  Scoring changes no result of the engine, and with no score running every launch sequence is what it was.
 *
 * One period of quadrotor b, with cur[b] its current slot (0 at the start) and len the length of its trajectory:
 *  1. A flight begins with a period whose step used cursor 0: if i == 0 and slot cur[b] already holds a period, cur[b] += 1.  No install
 *     path is hooked: a mission's install, mpcq_replan*, mpcq_replace_trajectories and mpcq_set_trajectories all open a slot this way
 *     (and so does mpcq_reset or mpcq_set_state(idx = 0): they are allowed while a score is running and show as a new flight, as they
 *     show in later rows of a recording).  A score started in mid-flight puts the partial flight into slot 0.
 *  2. If cur[b] >= F: overflow[b] += 1 and nothing else is written for this period (cur[b] stays at F).
 *  3. The period is a tail period iff i >= len - tail_rows.  tail_rows = 0: exactly the periods beyond the flight's last row (a quadrotor
 *     that holds its last reference row, or overshot without finishing); tail_rows = 100: the reference's dropped last second at 100 Hz rows.
 *  4. With ep = sum_k (x[k] - ref[k])^2, ev = sum_k (x[7+k] - ref[7+k])^2, v2 = sum_k x[7+k]^2, vr2 = sum_k ref[7+k]^2 over k = 0..2 the
 *     row of slot cur[b] is updated.  Every field starts at 0, except 12 and 13, which start at -1; counts are doubles and stay exact:
 *       #  name             updated in     value
 *       0  steps            non-tail       += 1
 *       1  sum_epos2        non-tail       += ep
 *       2  sum_evel2        non-tail       += ev
 *       3  max_epos2        non-tail       max(., ep)
 *       4  sum_rms_pos      non-tail       += sqrt(ep / 3)   (Visualiser's per-step rms_pos)
 *       5  max_v2           non-tail       max(., v2)
 *       6  max_vref2        non-tail       max(., vr2)
 *       7  sum_cost         non-tail       += cost[b]
 *       8  tail_steps       tail           += 1
 *       9  bad_status       every period   += (status != 0)
 *      10  fallbacks        every period   += (qp_iter / 1000 % 10 != 0)
 *      11  factorisations   every period   += qp_iter % 1000
 *      12  first_period     every period   set once: the period number (since mpcq_score_start / mpcq_score_clear) of the slot's first period
 *      13  last_period      every period   = the period number
 *      14  rows             every period   = len
 *      15  finished         every period   = 1 once the finished flag is set after a step of this flight
 * Quadrotors are independent and updated in period order on the stream of their group: the table does not depend on mpcq_tuning.groups.
 * A running score is not part of a checkpoint, and nothing is reduced across ranks (a score is per shard, as a recording is). */
#define MPCQ_SCORE_WIDTH 16
/* Starts a score with `flights` = F >= 1 slots per quadrotor (memory: B x F x 128 bytes) from the next period on; while one is running it
 * is replaced (table, slots and period count start again).  MPCQ_ERR_INVALID: flights < 1, tail_rows < 0, and a table of B x F x 16 >= 2^31
 * doubles (16 GiB: refused before anything is allocated, so that the element counts of the launches and of the copy stay within 32 bits).
 * MPCQ_ERR_STATE: before mpcq_set_trajectories.  mpcq_sim_run (one persistent launch) scores nothing: MPCQ_ERR_STATE while a score is
 * running. */
int mpcq_score_start(mpcq_engine* e, int32_t flights /*F >= 1 slots per quadrotor*/, int32_t tail_rows /*>= 0*/);
/* The table, behind everything the engine has enqueued on every group stream; every pointer may be NULL.  flights [B]: slots that hold
 * a period (0..F); overflow [B]: periods that found no slot; periods: periods counted since mpcq_score_start / mpcq_score_clear (per
 * quadrotor the sum over its slots of steps + tail_steps, plus overflow[b], equals it).  MPCQ_ERR_STATE: no score running. */
int mpcq_score_get(mpcq_engine* e, double* score /*[B,F,16] or NULL*/, int32_t* flights /*[B] or NULL: slots holding a period*/,
                   int32_t* overflow /*[B] or NULL*/, int64_t* periods /*or NULL: periods since score_start / score_clear*/);
/* table, cur, overflow and period count back to the start values; stays on.  MPCQ_ERR_STATE: no score running. */
int mpcq_score_clear(mpcq_engine* e);
/* off, buffers freed: period launches are exactly what they are without it.  MPCQ_ERR_STATE: no score running. */
int mpcq_score_stop(mpcq_engine* e);

/* ---- RGP read-out with uncertainty (since 0.6.4): GPEnsemble.predict(X_t, std=True) (src/gp/GPE.py:165-201) over RGP.predict
 * (src/gp/RGP.py:168-229) for every quadrotor and axis, evaluated on the device.  With the axis' basis X, theta = (L, sigma_f, sigma_n),
 * K_x^-1 as built at mpcq_create and the quadrotor's mu, C:
 *     k*_j = sigma_f^2 exp(-(x - X_j)^2 / (2 L^2))     J = k* K_x^-1     mean = J mu     var = sigma_f^2 - J k*^T + J C J^T
 * An engine created with MPCQ_FLAG_STATIC_GP answers with the static GP's posterior (src/gp/GP.py:135-179): the same mean and
 * var = sigma_f^2 - J k*^T; C is not read.  All of it in float64: MPCQ_PRECISION_F32 engines convert mu and C as mpcq_get_rgp does, so
 * the result is the formula applied to what mpcq_get_rgp returns.  var is returned as computed (rounding may leave a tiny negative
 * number); the standard deviation is the caller's square root.
 * xq [3,M] (per_quad = 0: one grid per axis, shared by the batch) or [B,3,M] (per_quad = 1: every quadrotor its own points).  Ordered
 * behind everything the engine has enqueued, on all of its streams: it sees the state after the last period.  Blocks until the
 * outputs are on the host; changes no engine state.  MPCQ_ERR_INVALID: xq NULL, both outputs NULL, M outside 1..4096, per_quad not
 * 0 / 1.  MPCQ_ERR_STATE: nb = 0.  Non-finite query points are no error (a NaN point gives NaN outputs). */
int mpcq_rgp_predict(mpcq_engine* e, const double* xq, int32_t M, int32_t per_quad,
                     double* mean /*[B,3,M] or NULL*/, double* var /*[B,3,M] or NULL*/);
/* The same evaluation (bit for bit: one routine serves both) for rows row0 .. row0 + nrows - 1 of the active recording and the quadrotors
 * of mpcq_record_start in the caller's order, read from the recorder's device buffers in place: nothing but the outputs travels to the
 * host.  The row window bounds the size of the host arrays.  MPCQ_ERR_STATE: no active recording, nb = 0.  MPCQ_ERR_INVALID:
 * MPCQ_RECORD_RGP_MU not recorded; var asked for without MPCQ_RECORD_RGP_C (MPCQ_FLAG_STATIC_GP engines need only the mean field);
 * a window outside the rows recorded so far (nrows < 1 included); the argument rules of mpcq_rgp_predict. */
int mpcq_record_predict(mpcq_engine* e, const double* xq /*[3,M]*/, int32_t M, int32_t row0, int32_t nrows,
                        double* mean /*[count,nrows,3,M] or NULL*/, double* var /*[count,nrows,3,M] or NULL*/);

/* ---- training from a recording or a sample stream: the reference's offline trainer of the recursive GP loops
 * RGP.regress over a whole dataset for a model with its own basis and hyper-parameters (src/gp/rgp_train.py:95-103); RGP.learn
 * (src/gp/RGP.py:332-505) is fed the same way.  Here one persistent launch runs one workgroup per (stream, axis) regressor over all T
 * samples of its stream, the regressor state in LDS from the first sample to the last (csrc/mpcq_train.hpp).  All of it in float64,
 * whatever the engine's precision (the recorder stores the drag field in double).
 *   MPCQ_TRAIN_REGRESS: the update of mpcq_rgp_regress (formula above mpcq_rgp_predict: J = k* K_x^-1,
 *       G = C J^T / (sigma_f^2 - J k*^T + J C J^T + sigma_n^2), mu += G (y - J mu), C -= G J C, not symmetrised) with fixed theta,
 *       from mu = 0, C = K(X,X) + sigma_n^2 I, K_x^-1 from the routine mpcq_create uses.
 *   MPCQ_TRAIN_LEARN:   the update of mpcq_learn_step, sample by sample (one routine serves both), from the start values of
 *       mpcq_learn_create: mu_g = 0, C_g = K_x, mu_eta = theta, C_eta = I, K_x^-1 by the learner's Gauss-Jordan rebuild.
 * nb = 0 trains the engine's own model (its basis, theta and device copy of K_x^-1; an MPCQ_FLAG_STATIC_GP engine has one too):
 * the mu, C of a REGRESS run load into any engine of that model with mpcq_set_state. */
#define MPCQ_TRAIN_REGRESS 1
#define MPCQ_TRAIN_LEARN   2
typedef struct mpcq_train_spec {
  int32_t mode;          /* MPCQ_TRAIN_REGRESS | MPCQ_TRAIN_LEARN */
  int32_t pair_next;     /* 0: sample t = (v_body[t], a_drag[t]), what the flying engine regressed on.
                            1: (v_body[t], a_drag[t+1]), T-1 samples: the pairing of the reference's offline loader
                               (src/gp/DataLoaderGP.py:92-97) */
  int32_t nb;            /* 0: the engine's own basis / theta / K_x^-1 (basis, theta must be NULL); else 1..64 */
  const double* basis;   /* [3, nb] */
  const double* theta;   /* [3, 3] initial (LEARN) or fixed (REGRESS) L, sigma_f, sigma_n */
} mpcq_train_spec;
/* host arrays, each may be NULL (not all): S streams in the caller's order */
typedef struct mpcq_train_out {
  double* mu;       /* [S,3,nb] */
  double* C;        /* [S,3,nb,nb] */
  double* mu_eta;   /* [S,3,3]      LEARN only */
  double* C_eta;    /* [S,3,3,3]    LEARN only */
  double* Kx_inv;   /* [S,3,nb,nb]  LEARN only: K_x^-1 of the learned hyper-parameters */
} mpcq_train_out;
/* Trains S x 3 regressors on caller samples v_body, a_drag [S,T,3] (axis d of stream s learns from v_body[s,:,d] -> a_drag[s,:,d]).
 * Ordered behind everything the engine has enqueued, on all of its streams; blocks until the outputs are on the host; changes no
 * engine or recorder state (scratch belongs to the engine and goes with mpcq_destroy).  MPCQ_ERR_INVALID: spec or out NULL, all
 * outputs NULL, mode not one of the two, nb outside 0..64, nb > 0 with basis or theta NULL, nb = 0 with either set, a length scale
 * <= 0 (or K_x not positive definite), S < 1, T < 1 (T < 2 with pair_next), a LEARN-only output in REGRESS mode, v_body or a_drag
 * NULL.  MPCQ_ERR_STATE: nb = 0 on an engine with nb = 0.  MPCQ_ERR_DEVICE: the scratch cannot be allocated, or the device offers less
 * LDS per workgroup than the smallest layout needs.  Non-finite samples are no error: the regressors that see one come back NaN,
 * the others are untouched. */
int mpcq_rgp_train(mpcq_engine* e, const mpcq_train_spec* spec, const double* v_body /*[S,T,3]*/, const double* a_drag /*[S,T,3]*/,
                   int32_t S, int32_t T, mpcq_train_out* out);
/* The same training (bit for bit: one routine serves both) on rows row0 .. row0 + nrows - 1 of the active recording's MPCQ_RECORD_DRAG
 * field, read from the recorder's device buffer in place: S = the recording's count, in the caller's order as for mpcq_record_predict,
 * T = nrows.  MPCQ_ERR_STATE: no active recording (and the rule above).  MPCQ_ERR_INVALID: MPCQ_RECORD_DRAG not recorded, a window
 * outside the rows recorded so far (nrows < 1, or < 2 with pair_next, included), the argument rules of mpcq_rgp_train. */
int mpcq_record_train(mpcq_engine* e, const mpcq_train_spec* spec, int32_t row0, int32_t nrows, mpcq_train_out* out);

/* ---- the fleet: every quadrotor its own plant.  Without it all B quadrotors of an engine fly the one Quadrotor3D of mpcq_config, in its
 * drag = True, payload = False corner.  The reference's plant knows more (src/quad.py): a per-rotor rotor_functionality (:86-87, used in
 * thrust :344 and torques :371), a payload_mass (:93-94, used at :353) and body-frame disturbance force and torque f_d, t_d
 * (one_step_forward / f_vel / f_rate, :166-190, :348-349, :375-377).  A fleet is a table of B such plants on the device; while one is set,
 * the plant update of every period is a launch of a kernel that integrates each quadrotor with its own row (csrc/mpcq_fleet.hpp).  The
 * CONTROLLER keeps the engine's model (mpcq_config): only the plant changes, so the mismatch is what the RGP has to learn -- a sweep over
 * mass, drag, payload, rotor faults and gusts is one batch, scored per flight (mpcq_score_*).  g stays the engine's.
 * With f = u * rotor_functionality * max_thrust (u clipped to [0, 1] first, as Quadrotor3D.update does), R the rotation of the attitude:
 *     dv = R ([0, 0, sum f] + a_drag_body(v) mass + f_d) / mass - [0, 0, g] - [0, 0, payload_mass g / mass]
 *     dr = (torques of f through y_f, -x_f, z_l_tau + t_d + gyroscopic term) / J
 * integrated by the reference's RK4 (:181-186), n_sub substeps of sim_dt per period.  f_d / mass, t_d / J, payload_mass g / mass and the
 * reciprocals of mass and J are formed once, at mpcq_fleet_set.  A row that equals the engine's own plant with payload 0, functionality
 * 1 and no disturbance gives bit for bit the engine's shared plant: every extra is then an exact * 1.0 or + 0.0. */
typedef struct mpcq_plant {              /* one quadrotor's Quadrotor3D; g stays the engine's */
  double mass, J[3], max_thrust, x_f[4], y_f[4], z_l_tau[4];
  double rotor_drag[3], aero_drag;       /* src/quad.py:79-89 */
  double payload_mass;                   /* a_payload = -payload_mass g / mass, z only, as src/quad.py:353 has it (its own TODO included) */
  double rotor_functionality[4];         /* f_thrust = u * functionality * max_thrust, in thrust AND torques (:344, :371); each in [0, 1] */
  double f_d[3], t_d[3];                 /* body-frame disturbance force [N] and torque [N m] (:348, :375-377) */
  int32_t d_from, d_to;                  /* f_d, t_d act in fleet periods d_from <= p < d_to; d_to <= d_from: never */
} mpcq_plant;
/* The fleet period p counts the plant updates the engine has made since period0 was set: one per control period of mpcq_sim_steps /
 * mpcq_sim_control_periods (the same p for every group of that period, see mpcq_tuning.groups) and one per mpcq_sim_plant_period.
 * mpcq_step / mpcq_step_device_async / mpcq_solve update no plant -- the caller owns it -- and are unaffected.  While a fleet is set every
 * plant update of mpcq_sim_steps is a launch of its own, behind the recorder's row, the black box and the score and in front of the mission launch (a
 * mission plans from the fleet plant's state).  mpcq_sim_run (one persistent launch with the shared plant fused in) flies no fleet:
 * MPCQ_ERR_STATE while one is set.  mpcq_reset keeps the table and the period, mpcq_destroy frees it.
 *
 * mpcq_fleet_set uploads plants [B] (plant_size = the caller's sizeof(mpcq_plant)); calling it again replaces the table.  period0 >= 0
 * sets the fleet period, -1 keeps it (0 if no fleet is set).  MPCQ_ERR_INVALID, with the engine left as it was and mpcq_last_error()
 * naming the quadrotor and the field: plants NULL, a plant_size that is not this library's, period0 < -1, a value that is not finite,
 * mass, J or max_thrust <= 0, a rotor functionality outside [0, 1]. */
int mpcq_fleet_set(mpcq_engine* e, const mpcq_plant* plants /*[B]*/, uint64_t plant_size, int64_t period0 /*>= 0 sets the fleet period; -1 keeps it (0 if none active)*/);
/* The table as it was set (exactly: the host's copy) and the fleet period.  MPCQ_ERR_STATE: no fleet set; MPCQ_ERR_INVALID: plant_size. */
int mpcq_fleet_get(mpcq_engine* e, mpcq_plant* plants /*[B] or NULL*/, uint64_t plant_size, int64_t* period /*or NULL*/);
/* back to the engine's shared plant; launches as before this change.  MPCQ_ERR_STATE: no fleet set. */
int mpcq_fleet_stop(mpcq_engine* e);

/* ---- the sensor: noise, bias, latency and dropout between the plant and the controller.  Without it the closed loop of mpcq_sim_steps
 * measures the identity: the step solves from the plant's own state, exactly and at once.  A sensor is a table of B mpcq_sensor on the
 * device; while one runs, one launch of a kernel of its own (csrc/mpcq_sensor.hpp) stands in front of every control period of
 * mpcq_sim_steps / mpcq_sim_control_periods and turns the true plant state into the measurement the step solves from.  The step kernel
 * takes its measurement by pointer and is untouched.  State x = [p(3), q(4, w first), v(3), r(3)]; sensor period n starts at period0;
 * quadrotor b has the global index i = index0 + b.
 *   Draws.  Philox4x32-10 (multipliers D2511F53 / CD9E8D57, key increments 9E3779B9 / BB67AE85), counter (n lo32, n hi32, i lo32, c), key
 * (seed lo32, seed hi32), c = 0..3.  A word w becomes u = (w + 0.5) 2^-32 (exact in double, never 0 or 1).  Calls c = 0, 1, 2 give the
 * normals z[4c .. 4c+3]: from the words (w0, w1) rho = sqrt(-2 ln u0), z = rho cos(6.283185307179586 u1), then rho sin(same); the words
 * (w2, w3) likewise.  Word 0 of call 3 is u_drop.  The draws depend on (seed, n, i) only: not on the batch, a shard, a group or the
 * order of launches.
 *   Sample m_n.  p, v, r: x + bias + sigma z with z[0:3], z[6:9], z[9:12].  Attitude: theta = bias_att + sigma_att z[3:6], a = |theta|,
 * q_m = normalise(q (x) [cos(a/2), sin(a/2) theta / a]) (the identity rotation for a = 0).  A channel (p, att, v, r) whose sigma and bias
 * are all zero is copied, not computed: an all-zero sensor is the identity bit for bit.
 *   Ring.  m_n goes to slot (n - period0) mod depth.
 *   Delivery.  The candidate is m_max(n - delay, period0).  A period is dropped if n > period0 and (u_drop < p_drop or out_from <= n <
 * out_to): the delivered measurement stays as it was and age += 1.  Otherwise delivered = candidate and age = min(delay, n - period0).
 * Both comparisons are exact, so the drop pattern is reproducible bit for bit.
 *   Who reads what.  The step, the recorder's rows, the black box's rows and the exploration read the measurement, as a real log would;
 * the step kernel's own tracking accumulators (mpcq_get_tracking_stats) too.  The mission plans from the true plant state.  The
 * scoreboard and the black box's judge read the measurement under MPCQ_SENSOR_JUDGE_MEASURED and the true plant state (mpcq_sim_get_state)
 * under MPCQ_SENSOR_JUDGE_TRUTH -- in every control period, those of mpcq_step / mpcq_step_device_async included.
 *   Period order with a sensor: sensor -> recorder / black box snapshots -> step -> rows -> score -> exploration -> plant -> mission.  Every
 * plant update of mpcq_sim_steps is a launch of its own then, as with a fleet.  mpcq_step / mpcq_step_device_async take the caller's
 * measurement and do not advance the sensor: a host loop is mpcq_sensor_sample -> mpcq_step -> mpcq_sim_plant_period, and flies bit for
 * bit what mpcq_sim_steps flies.  mpcq_sim_run (one persistent launch) measures through no sensor: MPCQ_ERR_STATE while one runs.
 * mpcq_reset and mpcq_sim_reset keep the table, the ring and the sensor period; mpcq_destroy frees them.  With no sensor started every
 * launch sequence is what it was.  Device memory: 104 (depth + 1) + 224 bytes per quadrotor. */
typedef struct mpcq_sensor {            /* one quadrotor's sensor; all zero = the identity */
  double sigma_p[3], sigma_att[3], sigma_v[3], sigma_r[3];  /* white noise per period, std dev; att: rotation vector [rad], body frame */
  double bias_p[3],  bias_att[3],  bias_v[3],  bias_r[3];   /* constant offsets */
  double p_drop;                        /* probability that a period delivers nothing, [0, 1] */
  int32_t delay;                        /* periods between sampling and delivery, 0 .. depth-1 */
  int32_t reserved;
  int64_t out_from, out_to;             /* outage: nothing delivered in sensor periods [out_from, out_to) */
} mpcq_sensor;
#define MPCQ_SENSOR_JUDGE_MEASURED 0    /* score and black box judge what the controller saw (what a real log holds) */
#define MPCQ_SENSOR_JUDGE_TRUTH    1    /* score launch and the black box's judge read the true plant state */
/* Start (or, while one runs, replace) the sensor: sensors [B] (sensor_size = the caller's sizeof(mpcq_sensor)), the seed of the draws,
 * the global index of quadrotor 0, the first sensor period, the depth of the ring (1..32) and who judges.  The ring starts empty, the
 * delivered measurement and age are zero until the first period.  MPCQ_ERR_INVALID, with the engine left as it was -- a running sensor
 * goes on delivering what it would have -- and mpcq_last_error() naming the quadrotor and the field: sensors NULL, a sensor_size that is
 * not this library's, a sigma that is negative or not finite, a bias that is not finite, p_drop outside [0, 1], delay outside
 * 0..depth-1, depth outside 1..32, an unknown judge, a negative period0 or index0.  MPCQ_ERR_DEVICE: the buffers cannot be allocated. */
int mpcq_sensor_start(mpcq_engine* e, const mpcq_sensor* sensors /*[B]*/, uint64_t sensor_size, uint64_t seed,
                      int64_t index0 /*global index of quadrotor 0*/, int64_t period0, int32_t depth /*1..32*/, int32_t judge);
/* The delivered measurement, its age in periods and the number of the NEXT sensor period, behind everything the engine has enqueued.
 * MPCQ_ERR_STATE: no sensor running. */
int mpcq_sensor_get(mpcq_engine* e, double* x_meas /*[B,13] or NULL*/, int32_t* age /*[B] or NULL*/, int64_t* period /*or NULL*/);
/* One sensor launch on the current plant state; advances the sensor period and returns the delivered measurement: for host loops of
 * mpcq_step + mpcq_sim_plant_period.  MPCQ_ERR_STATE: no sensor running; MPCQ_ERR_INVALID: x_meas NULL. */
int mpcq_sensor_sample(mpcq_engine* e, double* x_meas /*[B,13]*/);
/* Sensor off, buffers freed: the measurement is the identity again and period launches are what they are without it.  MPCQ_ERR_STATE:
 * no sensor running. */
int mpcq_sensor_stop(mpcq_engine* e);

/* ---- exploration: mission limits from each quadrotor's envelope.  The reference's exploration loop (src/explore_trajectories.py:59-125)
 * flies one flight, trains a GP on that run and asks Explorer (src/Explorer.py:23-84) how far the training inputs reach in body-frame
 * velocity; the next flight gets v_max = a_max = velocity_to_explore, each clipped at 30 (:67-78).  Here the RGP regresses every period,
 * so the samples a flight contributed are the v_body of its periods, and the rule runs on the device, per quadrotor, in the period a
 * flight ends: no host decides how fast the next leg of a mission is flown.
 *   Envelope.  env [B,3,2] holds min and max of v_body per axis, samples [B] how many periods it covers.  The sample of a period is
 * v_body = R(q)^T v of the measurement the period's step solved from -- bit for bit the first three entries of MPCQ_RECORD_DRAG.  With
 * samples == 0 the envelope reads min = max = 0 on every axis (Explorer's `gpe is None`, src/Explorer.py:70-74).
 *   Rule (one mpcq_explore_rule per quadrotor).  Over the axes of `axes` (bit i: axis i; 7: all three, the reference):
 * vabs = max(0, max, |min|) with the reference's strict comparisons (calculate_explored_vmax, src/Explorer.py:51-63), explored = the
 * smallest vabs, v = explored + step if that is < desired, else desired (calculate_velocity_to_explore, :40-48), v_max = min(v, v_limit),
 * a_max = min(v, a_limit) (src/explore_trajectories.py:67-78).  The reference's numbers: step 10, desired 20, limits 30.
 *   Policy.  Quadrotor b is due in a period when finished[b] != 0 && leg[b] < L; if leg_mask[b, leg[b]] != 0 the device writes v_max and
 * a_max of that leg into the mission's legs table before the mission launch of the same period plans it.  Kind and radius stay: a
 * circle leg flies its radius at the explored speed.  leg_limits [B,L,3] logs (explored, v_max, a_max) of every leg written so; NaN
 * where none was (not consumed yet, or not explored).
 *   Launch.  One launch per period and range of quadrotors, behind the step (and the recorder's row, the black box and the score), in front of the
 * plant and mission launches, on every period a mission runs on: mpcq_sim_steps (each group's range on its stream),
 * mpcq_sim_control_periods, mpcq_step, mpcq_step_device_async.  mpcq_sim_run: MPCQ_ERR_STATE, as for the mission.  With no exploration
 * started every launch sequence and result is what it was.
 *   Two deliberate differences from the reference: it takes the range of the 10 GMM-selected training samples of the run, this the range of
 * all samples of the flight; and the limits follow the sample range, not the RGP's posterior variance. */
#define MPCQ_EXPLORE_LAST_FLIGHT 0   /* the reference: every run trains a fresh GP -- the envelope restarts in the period whose step used cursor 0 (a new flight, as MPCQ_RECORD_SOLVER shows it) */
#define MPCQ_EXPLORE_CUMULATIVE  1   /* the envelope never restarts */
typedef struct mpcq_explore_rule { double step, desired, v_limit, a_limit; int32_t mode, axes; } mpcq_explore_rule;   /* one per quadrotor */
/* Start (or, while one runs, replace) the exploration of the mission that is set: rules [B] (rule_size = the caller's
 * sizeof(mpcq_explore_rule)), leg_mask [B,L] (NULL: every leg is explored), and the envelope to start from: env0 [B,3,2] with
 * samples0 [B] (what mpcq_explore_get returned: a checkpoint), or both NULL for the empty envelope.  leg_limits starts all NaN.
 * MPCQ_ERR_STATE: no mission set.  MPCQ_ERR_INVALID, with the engine left as it was and mpcq_last_error() naming the quadrotor: rules
 * NULL, a rule_size that is not this library's, step / desired / v_limit / a_limit not finite and > 0, mode not 0 or 1, axes outside
 * 1..7, exactly one of env0 / samples0 given, a negative samples0.
 * mpcq_mission_set, mpcq_mission_set_legs and mpcq_mission_stop end a running exploration: the table it writes into is gone. */
int mpcq_explore_start(mpcq_engine* e, const mpcq_explore_rule* rules /*[B]*/, uint64_t rule_size, const uint8_t* leg_mask /*[B,L] or NULL: every leg*/,
                       const double* env0 /*[B,3,2] or NULL*/, const int64_t* samples0 /*[B] or NULL*/);
/* Envelope, sample counts and the log, behind everything the engine has enqueued; any pointer may be NULL.  MPCQ_ERR_STATE: no
 * exploration running. */
int mpcq_explore_get(mpcq_engine* e, double* env /*[B,3,2]*/, int64_t* samples /*[B]*/, double* leg_limits /*[B,L,3]*/);
/* Exploration off: the mission flies the rest of its legs with the limits the table holds now (what was written stays written), period
 * launches are what they are without it.  MPCQ_ERR_STATE: no exploration running. */
int mpcq_explore_stop(mpcq_engine* e);

/* ---- RGP.learn (src/gp/RGP.py:332-505), SURVEY §8 f4: hyper-parameter learning of the recursive GP (unscented
 * transform over eta = (L, sigma_f, sigma_n) + Kalman / smoother updates) for batch x 3 independent (quadrotor, axis)
 * regressors on the device, fp64.  The loop body never calls learn in the reference (offline estimator), so this is an
 * object of its own: basis [3, nb] and theta [3, 3] as in mpcq_config (initial values, shared by the batch), nb <= 64.
 * mpcq_learn_step feeds one sample per regressor: v_body [B,3] (inputs), a_drag [B,3] (targets).  mpcq_learn_get:
 * mu_g [B,3,nb], C_g [B,3,nb,nb], mu_eta [B,3,3], C_eta [B,3,3,3], Kx_inv [B,3,nb,nb] (K_x^-1 rebuilt for the new
 * hyper-parameters, RGP.py:499-500); any pointer may be NULL.  Errors: mpcq_learn_last_error(). */
typedef struct mpcq_learner mpcq_learner;
const char* mpcq_learn_last_error(void);
int mpcq_learn_create(int32_t batch, int32_t nb, const double* basis, const double* theta, int32_t device, mpcq_learner** out);
int mpcq_learn_destroy(mpcq_learner* l);
int mpcq_learn_step(mpcq_learner* l, const double* v_body, const double* a_drag);
int mpcq_learn_get(mpcq_learner* l, double* mu_g, double* C_g, double* mu_eta, double* C_eta, double* Kx_inv);

#ifdef __cplusplus
}
#endif
#endif /* MPCQ_H */

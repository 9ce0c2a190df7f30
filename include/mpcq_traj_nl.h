/* mpcq_traj_nl.h — C ABI of libmpcq_traj.so, part 2 (since 0.6.2): the nonlinear stage of the min-snap generator (host code, C++).
 * Conventions as include/mpcq_traj.h (caller-owned, C-contiguous float64 arrays; wp [n,3], pieces [n-1,33]). */
#ifndef MPCQ_TRAJ_NL_H
#define MPCQ_TRAJ_NL_H
#include <stdint.h>
#include "mpcq_nl_options.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The nonlinear stage of the reference's generator (PolynomialOptimizationNonLinear<8> of mav_trajectory_generation, with nlopt's
 * Subplex), formulation rebuilt, optimiser written here: minimise over x = [T_1..T_{n-1}, d_free]
 *   f = J_d(T, d_free) + time_penalty (sum T)^2 (time_cost 1: time_penalty sum T)
 *       + min(cap, exp(w_s (vpk / v_max - 1))) + min(cap, exp(w_s (apk / a_max - 1)))     (dropped with use_soft_constraints = 0)
 * J_d the cost of mpcq_minsnap_from_derivatives, vpk / apk the peak speed / acceleration at the sample points of the generators' limit check
 * (dt 0.01; the library finds them by root finding -- a deliberate deviation).  Start: the linear stage (Nfabian times raised to 0.1 s, the
 * d_free that minimise J_d there); bounds 0.1 <= T <= 10 T_start, |velocity| <= v_max, |acceleration| <= a_max per component, jerk free; Subplex (Rowan
 * 1990) stopped by f_rel / x_rel / max_evaluations.  Options and defaults: include/mpcq_nl_options.h (mpcq_minsnap_nl_defaults
 * returns MPCQ_MINSNAP_NL_DEFAULTS).  Segment times are also bounded above by 10 x their start, and a flight whose linear stage lasts
 * longer than 300 s is refused (-3), so no evaluation samples more than 3 000 s of flight.  What is not
 * reproducible is nlopt's exact iterate path.  A NULL options pointer means the defaults. */
mpcq_minsnap_nl_options mpcq_minsnap_nl_defaults(void);
/* f at (T [n-1], d_free [n-2,3,3]) for derivative_to_optimize 2..4; parts [4] (may be NULL): derivative cost, time cost, soft speed term, soft
 * acceleration term.  Returns f, NaN on bad arguments (2 <= n <= 8, 0 < T <= 3000, limits > 0, options valid). */
double mpcq_minsnap_nl_objective(const double* wp, int32_t n, const double* T, const double* d_free, double v_max, double a_max,
                                 int32_t derivative_to_optimize, const mpcq_minsnap_nl_options* opts, double* parts);
/* The optimised flight: pieces [n-1,33]; d_free_out [n-2,3,3] (may be NULL); info [6] (may be NULL): f at the start, f at the end, evaluations
 * used, total duration, peak speed, peak acceleration (sampled; soft limits may be exceeded).  2 <= n <= 8.  Returns 0, -1 bad arguments,
 * -2 singular linear stage, -3 the linear stage lasts longer than 300 s. */
int mpcq_minsnap_nonlinear(const double* wp, int32_t n, double v_max, double a_max, int32_t derivative_to_optimize, const mpcq_minsnap_nl_options* opts,
                           double* pieces, double* d_free_out, double* info);

#ifdef __cplusplus
}
#endif
#endif /* MPCQ_TRAJ_NL_H */

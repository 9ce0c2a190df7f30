/* mpcq_nl_options.h — options of the min-snap generator's nonlinear stage, one definition for both C ABIs that take them:
 * include/mpcq_traj_nl.h (host library, mpcq_minsnap_nonlinear) and include/mpcq.h (device, mpcq_replan_nonlinear).
 * MPCQ_MINSNAP_NL_DEFAULTS is the one statement of the defaults: mav_trajectory_generation's published values as far as they can be stated
 * without its source (time_penalty 500, soft_constraint_weight 100, cap 1e12), nlopt's stopping rules of the reference's genTrajectory
 * (f_rel 0.05, x_rel 0.1, 1000 evaluations).  Valid: time_penalty finite and > 0 (with 0 nothing bounds the segment times from above
 * but the box), soft_constraint_weight finite and > 0, soft_constraint_cap > 0, f_rel / x_rel finite and >= 0, max_evaluations >= 1,
 * time_cost 1 or 2, use_soft_constraints 0 or 1. */
#ifndef MPCQ_NL_OPTIONS_H
#define MPCQ_NL_OPTIONS_H
#include <stdint.h>

typedef struct mpcq_minsnap_nl_options {
  double time_penalty;            /* w_t */
  double soft_constraint_weight;  /* w_s */
  double soft_constraint_cap;     /* cap of each soft term */
  double f_rel;                   /* stop when a Subplex cycle that moved x improves f by less than f_rel |f| */
  double x_rel;                   /* stop when every |step_i| <= x_rel |x_i| */
  int32_t max_evaluations;        /* exact cap on objective evaluations */
  int32_t time_cost;              /* 2: w_t (sum T)^2, 1: w_t sum T */
  int32_t use_soft_constraints;   /* 1 / 0 */
  int32_t reserved;               /* 0 */
} mpcq_minsnap_nl_options;

#define MPCQ_MINSNAP_NL_DEFAULTS {500.0, 100.0, 1e12, 0.05, 0.1, 1000, 2, 1, 0}

#ifdef __cplusplus
static_assert(sizeof(mpcq_minsnap_nl_options) == 56, "mpcq_minsnap_nl_options layout (mpc_quad_ros_amd/_lib.py NlOptions)");
#endif
#endif /* MPCQ_NL_OPTIONS_H */

// mpcq_replan_nl.hpp — device nonlinear min-snap generator (mpcq_replan_nonlinear).  Included from mpcq_api.hip after mpcq_replan.hpp.
//
// The device statement of csrc/minsnap.cpp's mpcq_minsnap_nonlinear + mpcq_minsnap_sample, one wavefront per selected quadrotor:
//  * the linear-stage start from mpcq::replan::unit_forms + solve_pieces (A(1)^-1, M(1) in LDS; the free derivatives at the Nfabian
//    times raised to 0.1 s), whose operations the host states in mpcq_nl::nl_unit_forms / nl_linear_dfree;
//  * the Subplex driver (mpcq_nl::sbx_next, the host's code) on lane 0, its state in LDS; the other lanes wait at the barrier;
//  * each evaluation spread over the lanes: T^k one (segment, power) per lane, coefficients and segment costs one (segment, axis) per
//    lane, the sum in the host's order (mpcq_nl::nl_total), peaks over the sample points one point per lane and a wave max;
//  * sampling into the slot and the install of mpcq_replan (slot_commit).
// Floating-point contraction is off (the shared functions switch it off themselves): the driver has to see the host's numbers.
#pragma once
#include "mpcq_minsnap_nl.hpp"

namespace mpcq {
namespace replan {

struct NlLds {
  Lds base;                     // V, T, Tp, A1i, M1, R, coef, ends, first / steps, last (mpcq_replan)
  mpcq_nl::Sbx sbx;
  double q[MAXS][3];            // segment costs of the evaluation
  double fval;
  int req;
};

// f at x (LDS, n = vertices); leaves coef / Tp / first / steps of x in S.base and the peaks in *vpk / *apk (every lane).  Wave-uniform.
__device__ inline double nl_evaluate(NlLds& L, const double* x, int n, int order, const mpcq_nl::Opts& o, double v_max, double a_max, double* vpk,
                                     double* apk) {
#pragma clang fp contract(off)
  Lds& S = L.base;
  const int lane = threadIdx.x, ns = n - 1;
  for (int it = lane; it < ns * 15; it += 64) {
    const int s = it / 15, k = it - s * 15 - 7;
    S.Tp[s][k + 7] = mpcq_nl::nl_ipow(x[s], k);
  }
  if (lane == 0) mpcq_nl::nl_grid(x, ns, S.first, S.steps);
  __syncthreads();
  if (lane < ns * 3) {
    const int s = lane / 3, ax = lane - s * 3;
    double d[8];
    mpcq_nl::nl_seg_d(S.V, n, x, s, ax, d);
    mpcq_nl::nl_seg_coef_cost(S.A1i, S.M1, S.Tp[s], d, order, S.coef[s][ax], &L.q[s][ax]);
  }
  __syncthreads();
  double vm = 0, am = 0;
  for (int j = lane; j < S.first[ns]; j += 64) {
    int s = 0;
    while (j >= S.first[s + 1]) ++s;
    double sv, sa;
    mpcq_nl::nl_sample_peak(S.coef[s], x[s], j - S.first[s], S.steps[s], &sv, &sa);
    vm = vm < sv ? sv : vm;
    am = am < sa ? sa : am;
  }
  vm = wave_max(vm); am = wave_max(am);
  *vpk = vm; *apk = am;
  return mpcq_nl::nl_total(L.q, ns, x, o, vm, am, v_max, a_max, nullptr);
}

// The nonlinear flight of one quadrotor, by the wavefront that calls it: planned through [p0, wp_b[0..n_wp)] and, on DONE, installed in slot b.
// Returns the MPCQ_REPLAN_* code (wave-uniform).  Optional outputs of this quadrotor: info [6], pieces [n_wp,33], dfree [n_wp-1,3,3] (NaN
// unless a flight was made).  Shared by replan_nl_kernel (a host call) and mission_kernel (mpcq_mission.hpp, behind a period).
__device__ inline int plan_nonlinear(NlLds& L, double* traj, int Tmax, int* lens, int* idx, int* finished, int b, const double* p0, const double* wp_b,
                                     int n_wp, double v_max, double a_max, int order, double dt, const mpcq_nl::Opts& o, double* info, double* pieces,
                                     double* dfree) {
#pragma clang fp contract(off)
  Lds& S = L.base;
  const int lane = threadIdx.x, n = n_wp + 1, ns = n_wp, nv = ns + 9 * (n - 2);
  auto finish = [&](int c, bool outputs) {   // result code; NaN outputs unless a flight was made
    if (outputs) return c;
    const double nan = __builtin_nan("");
    if (info && lane < 6) info[lane] = nan;
    if (pieces)
      for (int e = lane; e < ns * 33; e += 64) pieces[e] = nan;
    if (dfree)
      for (int e = lane; e < 9 * (n - 2); e += 64) dfree[e] = nan;
    return c;
  };
  if (!load_vertices(S, p0, wp_b, n_wp)) return finish(BAD_INPUT, false);
  // the linear stage: Nfabian times (shared nl_exp) raised to 0.1 s, the free derivatives that minimise J_d there
  if (lane < ns) S.T[lane] = mpcq_nl::nl_estimate_time(S.V, lane, v_max, a_max);
  unit_forms(S, order);   // (its barriers publish T)
  double total0 = 0;      // a linear stage longer than MAX_START_DURATION is refused (bounds every evaluation's work; the host's -3)
  for (int s = 0; s < ns; ++s) total0 = total0 + S.T[s];
  if (!(total0 <= mpcq_nl::MAX_START_DURATION)) return finish(LIMITS, false);
  if (!solve_pieces(S, n, order)) return finish(-2, false);
  if (lane == 0) {
    mpcq_nl::Sbx& X = L.sbx;
    double* x0 = X.xt;   // (staging: sbx_init copies it into X.x before X.xt is written again)
    for (int s = 0; s < ns; ++s) x0[s] = S.T[s];
    const int nf = 3 * (n - 2);
    for (int v = 0; v < n - 2; ++v)
      for (int ax = 0; ax < 3; ++ax)
        for (int r = 0; r < 3; ++r) x0[ns + (v * 3 + ax) * 3 + r] = S.R[3 * v + r][nf + ax];
    mpcq_nl::nl_box(n, v_max, a_max, x0, X.dx, X.xprev, X.step);   // (lo / hi staged in dx / xprev)
    mpcq_nl::sbx_init(X, nv, x0, X.step, X.dx, X.xprev, o.f_rel, o.x_rel, o.max_evaluations);
    L.fval = 0.0;
  }
  __syncthreads();
  double vpk, apk;
  for (;;) {
    if (lane == 0) L.req = mpcq_nl::sbx_next(L.sbx, L.fval);
    __syncthreads();
    if (!L.req) break;
    const double f = nl_evaluate(L, L.sbx.xt, n, order, o, v_max, a_max, &vpk, &apk);
    if (lane == 0) L.fval = f;
    __syncthreads();
  }
  nl_evaluate(L, L.sbx.x, n, order, o, v_max, a_max, &vpk, &apk);   // pieces and peaks of the result (not counted)
  const double* x = L.sbx.x;
  double total = 0;
  for (int s = 0; s < ns; ++s) total = total + x[s];
  if (info && lane == 0) {
    double* r = info;
    r[0] = L.sbx.f0; r[1] = L.sbx.f; r[2] = L.sbx.nev; r[3] = total; r[4] = vpk; r[5] = apk;
  }
  if (pieces)
    for (int e = lane; e < ns * 33; e += 64) {
      const int s = e / 33, c = e - s * 33;
      pieces[e] = c == 0 ? x[s] : (c < 25 ? S.coef[s][(c - 1) / NC][(c - 1) % NC] : 0.0);
    }
  if (dfree)
    for (int e = lane; e < 9 * (n - 2); e += 64) dfree[e] = x[ns + e];
  // sampling (mpcq_minsnap_sample) and install, as replan_kernel
  const double q = ceil(total / dt);   // (compared before the conversion: total / dt need not fit an int)
  if (!(q <= (double)Tmax)) return finish(TOO_LONG, true);
  const int rows = (int)q;
  if (lane == 0) {
    double e = 0;
    for (int s = 0; s < ns; ++s) { e = e + x[s]; S.ends[s] = e; }
  }
  __syncthreads();
  sample_install(S, traj, Tmax, lens, idx, finished, b, ns, rows, dt);
  return finish(DONE, true);
}

// One workgroup (one wavefront) per quadrotor, arguments as replan_kernel plus the options and the optional outputs info [B,6],
// pieces [B,n_wp,33], d_free [B,n_wp-1,3,3] (NaN rows for quadrotors without a new flight).
__global__ __launch_bounds__(64) void replan_nl_kernel(double* traj, int Tmax, int* lens, int* idx, int* finished, const double* start, int start_stride,
                                                       const double* wp, int n_wp, double v_max, double a_max, int order, double dt,
                                                       const int* mask, int* code, mpcq_nl::Opts o, double* info, double* pieces, double* dfree) {
  NlLds& L = *reinterpret_cast<NlLds*>(smem_raw);
  const int b = blockIdx.x, lane = threadIdx.x;
  double* info_b = info ? info + (size_t)b * 6 : nullptr;
  double* pieces_b = pieces ? pieces + (size_t)b * n_wp * 33 : nullptr;
  double* dfree_b = dfree ? dfree + (size_t)b * 9 * (n_wp - 1) : nullptr;
  const bool sel = mask ? mask[b] != 0 : finished[b] != 0;
  int c = SKIPPED;
  if (sel)
    c = plan_nonlinear(L, traj, Tmax, lens, idx, finished, b, start + (size_t)b * start_stride, wp + (size_t)b * n_wp * 3, n_wp, v_max, a_max, order, dt, o,
                       info_b, pieces_b, dfree_b);
  else {   // NaN rows
    const double nan = __builtin_nan("");
    if (info_b && lane < 6) info_b[lane] = nan;
    if (pieces_b)
      for (int e = lane; e < n_wp * 33; e += 64) pieces_b[e] = nan;
    if (dfree_b)
      for (int e = lane; e < 9 * (n_wp - 1); e += 64) dfree_b[e] = nan;
  }
  if (lane == 0) code[b] = c;
}

}  // namespace replan
}  // namespace mpcq

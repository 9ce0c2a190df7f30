// mpcq_minsnap_nl.hpp — the nonlinear stage of the min-snap generator, written once for the host library (minsnap.cpp:
// mpcq_minsnap_nonlinear, mpcq_minsnap_nl_objective) and the device (mpcq_replan_nl.hpp: mpcq_replan_nonlinear).
//
// Variables x = [T_1..T_m, d_free] (m = n - 1 segment times; d_free [n-2][3 axes][3] = velocity, acceleration, jerk at the interior
// vertices, the layout of mpcq_minsnap_from_derivatives).  Objective:
//   f(x) = J_d(T, d_free) + w_t (sum T)^2 [or w_t sum T] + min(cap, exp(w_s (vpk / v_max - 1))) + min(cap, exp(w_s (apk / a_max - 1)))
// with vpk / apk the peaks at the sample points of the host's `limits` (dt 0.01).  Minimised by Subplex (Rowan 1990), implemented
// here from its description as a reverse-communication state machine: sbx_next() either asks for f at S.xt or reports the end.
// The caller evaluates -- on the host in a loop, on the device spread over the lanes of one wavefront -- so the driver's control
// flow is plain scalar code that both sides run on the same numbers.
//
// Everything here is plain scalar arithmetic (+ - * / sqrt, floor / ceil, exact power-of-two scaling) with contraction off: the
// host library is built with -ffp-contract=off and every function below switches it off for the device compiler, so host and
// device evaluate the same function bit for bit.  nl_exp is this file's own exp for the same reason (libm and the device math
// library differ in the last bits, and one flipped comparison sends a simplex down another path).
#pragma once
#include <cmath>

#include "../../include/mpcq_nl_options.h"

#if defined(__HIP__)
#define MPCQ_HD __host__ __device__
#else
#define MPCQ_HD
#endif
#if defined(__clang__)
#define MPCQ_NL_NOCONTRACT _Pragma("clang fp contract(off)")
#else
#define MPCQ_NL_NOCONTRACT
#endif

namespace mpcq_nl {

constexpr int NC = 8, MAXV = 8, MAXS = MAXV - 1, MAXF = 3 * (MAXV - 2), RW = MAXF + 3;   // as mpcq::replan
constexpr int NV = MAXS + 9 * (MAXV - 2);   // variables: 7 times + 54 derivatives = 61
constexpr int KMAX = 5;                     // largest subspace (nsmax)
constexpr double PSI = 0.25, OMEGA = 0.1;   // Subplex: simplex reduction per subspace run, step rescale clamp
constexpr double T_MIN = 0.1, DT_LIM = 0.01;
// Upper bounds that keep every evaluation's work finite: T_i <= T_HI_FACTOR x its start (the box), a start of at most MAX_START_DURATION
// seconds (longer linear stages are refused), hence no evaluation samples more than T_MAX = 3 000 s of flight (300 000 points).
constexpr double T_HI_FACTOR = 10.0, MAX_START_DURATION = 300.0, T_MAX = T_HI_FACTOR * MAX_START_DURATION;

// the options of include/mpcq_nl_options.h, as the shared code sees them
struct Opts {
  double time_penalty, soft_weight, soft_cap, f_rel, x_rel;
  int max_evaluations, time_cost, use_soft_constraints;
};

// from the C struct; NULL: MPCQ_MINSNAP_NL_DEFAULTS
inline Opts nl_opts_from(const mpcq_minsnap_nl_options* p) {
  const mpcq_minsnap_nl_options d = MPCQ_MINSNAP_NL_DEFAULTS, &o = p ? *p : d;
  return {o.time_penalty, o.soft_constraint_weight, o.soft_constraint_cap, o.f_rel, o.x_rel, o.max_evaluations, o.time_cost, o.use_soft_constraints};
}

// the validity rules of include/mpcq_nl_options.h
inline bool nl_opts_valid(const Opts& o) {
  return std::isfinite(o.time_penalty) && o.time_penalty > 0 && std::isfinite(o.soft_weight) && o.soft_weight > 0 && o.soft_cap > 0 &&
         std::isfinite(o.f_rel) && o.f_rel >= 0 && std::isfinite(o.x_rel) && o.x_rel >= 0 && o.max_evaluations >= 1 &&
         (o.time_cost == 1 || o.time_cost == 2) && (o.use_soft_constraints == 0 || o.use_soft_constraints == 1);
}

// exp(x) from + - * / and ldexp: k = round(x / ln 2), r = x - k ln 2 (Cody-Waite, ln 2 split so that k ln2_hi is exact),
// exp(r) by its Taylor series to r^13 (|r| <= 0.35: truncation < 1e-17 relative), times 2^k.  Within ~2 ulp of exp.
MPCQ_HD inline double nl_exp(double x) {
  MPCQ_NL_NOCONTRACT
  if (!(x == x)) return x;
  if (x > 709.0) return HUGE_VAL;
  if (x < -708.0) return 0.0;
  const double k = floor(x * 1.4426950408889634 + 0.5);
  const double r = (x - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10;
  const double c[14] = {1.0, 1.0, 1.0 / 2, 1.0 / 6, 1.0 / 24, 1.0 / 120, 1.0 / 720, 1.0 / 5040, 1.0 / 40320, 1.0 / 362880,
                        1.0 / 3628800, 1.0 / 39916800, 1.0 / 479001600, 1.0 / 6227020800.0};
  double p = c[13];
  for (int i = 12; i >= 0; --i) p = p * r + c[i];
  return ldexp(p, (int)k);
}

MPCQ_HD inline double nl_ipow(double t, int k) {   // t^k for |k| <= 7 (mpcq::replan::ipow)
  MPCQ_NL_NOCONTRACT
  double r = 1.0;
  const int a = k < 0 ? -k : k;
  for (int i = 0; i < a; ++i) r *= t;
  return k < 0 ? 1.0 / r : r;
}

// Nfabian segment-time estimate of segment s (mpcq_minsnap_estimate_times with nl_exp), raised to the lower bound T_MIN
MPCQ_HD inline double nl_estimate_time(const double (*V)[3], int s, double v_max, double a_max) {
  MPCQ_NL_NOCONTRACT
  double d2 = 0;
  for (int k = 0; k < 3; ++k) d2 += (V[s + 1][k] - V[s][k]) * (V[s + 1][k] - V[s][k]);
  const double d = sqrt(d2), t = 2.0 * d / v_max * (1.0 + 6.5 * v_max / a_max * nl_exp(-2.0 * d / v_max));
  const double t1 = t > 1e-3 ? t : 1e-3;
  return t1 > T_MIN ? t1 : T_MIN;
}

// A(1)^-1 and M(1) of `order` -- the host's statement of mpcq::replan::unit_forms (same elimination, same M(1) sums)
inline void nl_unit_forms(int order, double (*A1i)[NC], double (*M1)[NC]) {
  MPCQ_NL_NOCONTRACT
  double A[NC][NC];
  for (int r = 0; r < 4; ++r)
    for (int i = 0; i < NC; ++i) {
      double f = 1;
      for (int k = 0; k < r; ++k) f *= (i - k);
      A[r][i] = i == r ? f : 0.0;
      A[4 + r][i] = i < r ? 0.0 : f;
    }
  for (int i = 0; i < NC; ++i)
    for (int j = 0; j < NC; ++j) A1i[i][j] = i == j ? 1.0 : 0.0;
  for (int c = 0; c < NC; ++c) {
    int p = c;
    for (int r = c + 1; r < NC; ++r)
      if (fabs(A[r][c]) > fabs(A[p][c])) p = r;
    if (p != c)
      for (int k = 0; k < NC; ++k) { const double t = A[p][k]; A[p][k] = A[c][k]; A[c][k] = t; const double u = A1i[p][k]; A1i[p][k] = A1i[c][k]; A1i[c][k] = u; }
    const double inv = 1.0 / A[c][c];
    for (int r = c + 1; r < NC; ++r) {
      const double f = A[r][c] * inv;
      if (f == 0.0) continue;
      for (int k = c; k < NC; ++k) A[r][k] -= f * A[c][k];
      for (int k = 0; k < NC; ++k) A1i[r][k] -= f * A1i[c][k];
    }
  }
  for (int c = NC - 1; c >= 0; --c)
    for (int k = 0; k < NC; ++k) {
      double s = A1i[c][k];
      for (int j = c + 1; j < NC; ++j) s -= A[c][j] * A1i[j][k];
      A1i[c][k] = s / A[c][c];
    }
  for (int a = 0; a < NC; ++a)
    for (int b = 0; b < NC; ++b) {
      double s = 0;
      for (int i = order; i < NC; ++i)
        for (int j = order; j < NC; ++j) {
          double fi = 1, fj = 1;
          for (int k = 0; k < order; ++k) fi *= (i - k);
          for (int k = 0; k < order; ++k) fj *= (j - k);
          s += A1i[i][a] * (fi * fj / (i + j - 2 * order + 1)) * A1i[j][b];
        }
      M1[a][b] = s;
    }
}

// The linear stage's free derivatives at times T: the host's statement of mpcq::replan::solve_pieces (the same assembly, the same
// elimination with partial pivoting on the system the three axes share, the same back substitution).  R [MAXF][RW] is workspace;
// dfree [n-2][3][3].  false if singular.
inline bool nl_linear_dfree(const double (*V)[3], int n, const double* T, const double (*M1)[NC], int order, double (*R)[RW], double* dfree) {
  MPCQ_NL_NOCONTRACT
  const int ns = n - 1, nf = 3 * (n - 2);
  double Tp[MAXS][15];
  for (int s = 0; s < ns; ++s)
    for (int k = -7; k <= 7; ++k) Tp[s][k + 7] = nl_ipow(T[s], k);
  auto free_idx = [&](int v, int r) { return (v == 0 || v == n - 1 || r == 0) ? -1 : 3 * (v - 1) + (r - 1); };
  auto M = [&](int s, int a, int b) { return M1[a][b] * Tp[s][(a & 3) + (b & 3) - 2 * order + 1 + 7]; };
  for (int fa = 0; fa < nf; ++fa)
    for (int fb = 0; fb < nf; ++fb) {
      const int va = fa / 3 + 1, ra = fa % 3 + 1, vb = fb / 3 + 1, rb = fb % 3 + 1;
      double acc = 0.0;
      const int s0 = (va > vb ? va : vb) - 1, s1 = va < vb ? va : vb;
      for (int s = s0; s <= s1; ++s)
        if (s >= 0 && s < ns) acc += M(s, (va - s) * 4 + ra, (vb - s) * 4 + rb);
      R[fa][fb] = acc;
    }
  for (int fa = 0; fa < nf; ++fa)
    for (int ax = 0; ax < 3; ++ax) {
      const int va = fa / 3 + 1, ra = fa % 3 + 1;
      double acc = 0.0;
      for (int s = va - 1; s <= va; ++s) {
        if (s < 0 || s >= ns) continue;
        const int a = (va - s) * 4 + ra;
        for (int b = 0; b < 2 * 4; ++b) {
          const int vb = s + b / 4, rb = b % 4;
          if (free_idx(vb, rb) >= 0) continue;
          acc -= M(s, a, b) * (rb == 0 ? V[vb][ax] : 0.0);
        }
      }
      R[fa][nf + ax] = acc;
    }
  for (int c = 0; c < nf; ++c) {
    double best = -1.0;
    int p = c;
    for (int r = c; r < nf; ++r)
      if (fabs(R[r][c]) > best) { best = fabs(R[r][c]); p = r; }
    if (!(best > 0.0)) return false;
    if (p != c)
      for (int k = 0; k < nf + 3; ++k) { const double t = R[p][k]; R[p][k] = R[c][k]; R[c][k] = t; }
    for (int r = c + 1; r < nf; ++r) {
      const double f = R[r][c] * (1.0 / R[c][c]);
      if (f != 0.0) {
        for (int k = c; k < nf; ++k) R[r][k] -= f * R[c][k];
        for (int k = 0; k < 3; ++k) R[r][nf + k] -= f * R[c][nf + k];
      }
    }
  }
  for (int ax = 0; ax < 3; ++ax)
    for (int c = nf - 1; c >= 0; --c) {
      double s = R[c][nf + ax];
      for (int j = c + 1; j < nf; ++j) s -= R[c][j] * R[j][nf + ax];
      R[c][nf + ax] = s / R[c][c];
    }
  for (int v = 0; v < n - 2; ++v)
    for (int ax = 0; ax < 3; ++ax)
      for (int r = 0; r < 3; ++r) dfree[(v * 3 + ax) * 3 + r] = R[3 * v + r][nf + ax];
  return true;
}

// ---- the objective, in pieces that the device spreads over its lanes

// box of x (T in [T_MIN, T_HI_FACTOR T_start], velocity / acceleration components within the limits, jerk free) and the initial Subplex
// step (0.1 |x_i|, floored at 0.01 s / 0.01 v_max / 0.01 a_max so that no step is 0); x = the start
MPCQ_HD inline void nl_box(int n, double v_max, double a_max, const double* x, double* lo, double* hi, double* step) {
  MPCQ_NL_NOCONTRACT
  const int m = n - 1;
  for (int i = 0; i < m + 9 * (n - 2); ++i) {
    const int r = i < m ? -1 : (i - m) % 3;   // -1 time, 0 velocity, 1 acceleration, 2 jerk
    const double lim = r == 0 ? v_max : (r == 1 ? a_max : HUGE_VAL);
    lo[i] = r < 0 ? T_MIN : -lim;
    hi[i] = r < 0 ? T_HI_FACTOR * x[i] : lim;
    const double floor_ = r < 0 ? 0.01 : 0.01 * (r == 0 ? v_max : a_max), s = 0.1 * fabs(x[i]);
    step[i] = s > floor_ ? s : floor_;
  }
}

// the 2 x 4 vertex values (p, v, a, j at both ends) of segment s, axis ax
MPCQ_HD inline void nl_seg_d(const double (*V)[3], int n, const double* x, int s, int ax, double* d) {
  const int m = n - 1;
  for (int a = 0; a < 8; ++a) {
    const int v = s + a / 4, r = a % 4;
    d[a] = r == 0 ? V[v][ax] : ((v == 0 || v == n - 1) ? 0.0 : x[m + ((v - 1) * 3 + ax) * 3 + (r - 1)]);
  }
}

// coefficients c = A(T)^-1 d = A(1)^-1_ia T^(r_a - i) d_a and the segment's cost q = d' M(T) d, M(T)_ab = M(1)_ab T^(r_a + r_b - 2 order + 1);
// Tp[k + 7] = T^k
MPCQ_HD inline void nl_seg_coef_cost(const double (*A1i)[NC], const double (*M1)[NC], const double* Tp, const double* d, int order, double* c, double* q) {
  MPCQ_NL_NOCONTRACT
  for (int i = 0; i < NC; ++i) {
    double acc = 0;
    for (int a = 0; a < 8; ++a) acc += A1i[i][a] * Tp[(a & 3) - i + 7] * d[a];
    c[i] = acc;
  }
  double J = 0;
  for (int a = 0; a < 8; ++a)
    for (int b = 0; b < 8; ++b) J += d[a] * (M1[a][b] * Tp[(a & 3) + (b & 3) - 2 * order + 1 + 7]) * d[b];
  *q = J;
}

// sample points of the host's `limits`: max(2, ceil(T_s / 0.01)) intervals per segment; first[s] = index of the first one.
// Callers keep T_s <= T_MAX (the box, the start guard, the objective's argument check), so the counts fit an int.
MPCQ_HD inline void nl_grid(const double* T, int ns, int* first, int* steps) {
  first[0] = 0;
  for (int s = 0; s < ns; ++s) {
    const double q = ceil(T[s] / DT_LIM);
    steps[s] = q > 2.0 ? (int)q : 2;
    first[s + 1] = first[s] + steps[s] + 1;
  }
}

// speed and acceleration magnitude at sample k of a segment with coefficients c[3][NC] (the host's `limits`)
MPCQ_HD inline void nl_sample_peak(const double (*c)[NC], double Ts, int k, int steps, double* sv, double* sa) {
  MPCQ_NL_NOCONTRACT
  const double t = Ts * k / steps;
  double v[3], a[3];
  for (int ax = 0; ax < 3; ++ax) {
    double vv = 0, aa = 0;
    for (int i = NC - 1; i >= 1; --i) vv = vv * t + i * c[ax][i];
    for (int i = NC - 1; i >= 2; --i) aa = aa * t + (double)i * (i - 1) * c[ax][i];
    v[ax] = vv; a[ax] = aa;
  }
  *sv = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  *sa = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
}

// f from the segment costs q[s][3], the times and the peaks.  Summation order: J = sum over axes (x, y, z) of the sum over segments.
// parts (may be NULL): derivative cost, time cost, soft speed term, soft acceleration term.
MPCQ_HD inline double nl_total(const double (*q)[3], int ns, const double* T, const Opts& o, double vpk, double apk, double v_max, double a_max,
                               double* parts) {
  MPCQ_NL_NOCONTRACT
  double J = 0;
  for (int ax = 0; ax < 3; ++ax) {
    double Ja = 0;
    for (int s = 0; s < ns; ++s) Ja += q[s][ax];
    J += Ja;
  }
  double ST = 0;
  for (int s = 0; s < ns; ++s) ST += T[s];
  const double tc = o.time_cost == 1 ? o.time_penalty * ST : o.time_penalty * (ST * ST);
  double sv = 0, sa = 0;
  if (o.use_soft_constraints) {
    sv = nl_exp(o.soft_weight * (vpk / v_max - 1.0));
    sa = nl_exp(o.soft_weight * (apk / a_max - 1.0));
    sv = sv < o.soft_cap ? sv : o.soft_cap;
    sa = sa < o.soft_cap ? sa : o.soft_cap;
  }
  if (parts) { parts[0] = J; parts[1] = tc; parts[2] = sv; parts[3] = sa; }
  return ((J + tc) + sv) + sa;
}

// ---- Subplex (Rowan 1990) as a reverse-communication state machine
//  * each cycle orders the coordinates by |dx| of the last cycle (|step| on the first), largest first (stable), and partitions them
//    into subspaces of nsmin = min(2, n) .. nsmax = min(5, n) coordinates, each next size chosen by Rowan's goodness
//    |dx|-mean(inside) - |dx|-mean(rest) (the smallest size among equals), subject to the rest remaining partitionable;
//  * Nelder-Mead on each subspace in turn (reflection 1, expansion 2, contraction 0.5, shrink 0.5), from the current point and its
//    step components; a run ends when the simplex size sum_j ||v_j - v_best||_1 has fallen to PSI times its initial size;
//  * then step *= ||dx||_1 / ||step||_1 clamped to [OMEGA, 1 / OMEGA] (PSI with a single subspace); components with dx != 0 take
//    dx's sign, the others flip;
//  * stops: a cycle that moved x improved f by less than f_rel |f|; every |step_i| <= x_rel |x_i|; the evaluation budget (checked
//    before every evaluation).  A cycle that found nothing better (dx = 0) does not count as converged: its step shrinks instead.
// Points leaving the box [lo, hi] are projected onto it.
enum : int { P_START, P_GOT_X0, P_CYCLE, P_SUB, P_INIT_V, P_ITER, P_REFL, P_EXPD, P_CONT_OUT, P_CONT_IN, P_SHRINK_NEXT, P_SHRINK_GOT, P_END_SUB,
             P_END_CYCLE, P_DONE };

struct Sbx {
  int n, nev, maxev, phase, cycle, nsub, isub, start, k, jv, nvalid, il, ih, is;
  double f, f0, fprev, fr, size0, frel, xrel;
  double x[NV], step[NV], dx[NV], xprev[NV], lo[NV], hi[NV], xt[NV];
  int perm[NV], sizes[NV];
  double simp[KMAX + 1][KMAX], fs[KMAX + 1], cen[KMAX], y[KMAX], yr[KMAX];
};

MPCQ_HD inline double nl_clamp(const Sbx& S, int i, double v) { return v < S.lo[i] ? S.lo[i] : (v > S.hi[i] ? S.hi[i] : v); }

MPCQ_HD inline void sbx_init(Sbx& S, int n, const double* x0, const double* step0, const double* lo, const double* hi, double f_rel, double x_rel,
                             int maxev) {
  S.n = n; S.nev = 0; S.maxev = maxev; S.phase = P_START; S.frel = f_rel; S.xrel = x_rel;
  for (int i = 0; i < n; ++i) {
    S.lo[i] = lo[i]; S.hi[i] = hi[i];
    S.x[i] = nl_clamp(S, i, x0[i]);
    S.step[i] = step0[i];
  }
}

// point with the current subspace's coordinates replaced by y -> S.xt (counted); false when the budget is spent
MPCQ_HD inline bool sbx_request(Sbx& S, const double* y, int next) {
  if (S.nev >= S.maxev) return false;
  for (int i = 0; i < S.n; ++i) S.xt[i] = S.x[i];
  if (y)
    for (int j = 0; j < S.k; ++j) S.xt[S.perm[S.start + j]] = y[j];
  ++S.nev;
  S.phase = next;
  return true;
}

MPCQ_HD inline void sbx_take_best(Sbx& S) {   // best evaluated vertex of the subspace run -> x, f
  int b = 0;
  for (int j = 1; j < S.nvalid; ++j)
    if (S.fs[j] < S.fs[b]) b = j;
  for (int j = 0; j < S.k; ++j) S.x[S.perm[S.start + j]] = S.simp[b][j];
  S.f = S.fs[b];
}

MPCQ_HD inline double sbx_size(const Sbx& S, int il) {
  MPCQ_NL_NOCONTRACT
  double sz = 0;
  for (int j = 0; j <= S.k; ++j)
    if (j != il)
      for (int d = 0; d < S.k; ++d) sz += fabs(S.simp[j][d] - S.simp[il][d]);
  return sz;
}

// Feed f at the last requested point (ignored on the first call).  Returns 1 if f is wanted at S.xt, 0 when done (S.x, S.f: result).
MPCQ_HD inline int sbx_next(Sbx& S, double fv) {
  MPCQ_NL_NOCONTRACT
  const int n = S.n, nsmin = n < 2 ? n : 2, nsmax = n < KMAX ? n : KMAX;
  for (;;) {
    switch (S.phase) {
      case P_START:
        S.k = 0;
        if (!sbx_request(S, nullptr, P_GOT_X0)) { S.phase = P_DONE; S.f = S.f0 = HUGE_VAL; break; }
        return 1;
      case P_GOT_X0:
        S.f = S.f0 = fv; S.cycle = 0;
        for (int i = 0; i < n; ++i) S.dx[i] = S.step[i];
        S.phase = P_CYCLE;
        break;
      case P_CYCLE: {
        S.fprev = S.f;
        for (int i = 0; i < n; ++i) { S.xprev[i] = S.x[i]; S.perm[i] = i; }
        for (int i = 1; i < n; ++i) {   // stable insertion sort by |dx| descending
          const int p = S.perm[i];
          int j = i;
          while (j > 0 && fabs(S.dx[S.perm[j - 1]]) < fabs(S.dx[p])) { S.perm[j] = S.perm[j - 1]; --j; }
          S.perm[j] = p;
        }
        S.nsub = 0;
        for (int pos = 0; pos < n;) {
          const int rem = n - pos;
          int bk = -1;
          double bg = 0;
          for (int k = nsmin; k <= (nsmax < rem ? nsmax : rem); ++k) {
            const int r2 = rem - k;
            if (r2 != 0 && (r2 < nsmin || ((r2 + nsmax - 1) / nsmax) * nsmin > r2)) continue;
            double s1 = 0, s2 = 0;
            for (int j = 0; j < k; ++j) s1 += fabs(S.dx[S.perm[pos + j]]);
            for (int j = k; j < rem; ++j) s2 += fabs(S.dx[S.perm[pos + j]]);
            const double g = s1 / k - (r2 ? s2 / r2 : 0.0);
            if (bk < 0 || g > bg) { bk = k; bg = g; }
          }
          if (bk < 0) bk = nsmax < rem ? nsmax : rem;
          S.sizes[S.nsub++] = bk;
          pos += bk;
        }
        S.isub = 0; S.start = 0;
        S.phase = P_SUB;
        break;
      }
      case P_SUB:
        S.k = S.sizes[S.isub];
        for (int j = 0; j < S.k; ++j) S.simp[0][j] = S.x[S.perm[S.start + j]];
        S.fs[0] = S.f; S.nvalid = 1; S.jv = 1;
        S.phase = P_INIT_V;
        // fall through: request vertex 1
      case P_INIT_V:
        if (S.phase == P_INIT_V && S.jv > 1) { S.fs[S.jv - 1] = fv; S.nvalid = S.jv; }
        if (S.jv <= S.k) {
          for (int j = 0; j < S.k; ++j) S.simp[S.jv][j] = S.simp[0][j];
          const int c = S.perm[S.start + S.jv - 1];
          S.simp[S.jv][S.jv - 1] = nl_clamp(S, c, S.simp[0][S.jv - 1] + S.step[c]);
          const int jv = S.jv++;
          S.phase = P_INIT_V;
          if (!sbx_request(S, S.simp[jv], P_INIT_V)) { S.jv = jv; sbx_take_best(S); S.phase = P_DONE; break; }
          return 1;
        }
        S.nvalid = S.k + 1;
        {
          int il = 0;
          for (int j = 1; j <= S.k; ++j)
            if (S.fs[j] < S.fs[il]) il = j;
          S.size0 = sbx_size(S, il);
        }
        S.phase = P_ITER;
        break;
      case P_ITER: {
        int il = 0, ih = 0;
        for (int j = 1; j <= S.k; ++j) {
          if (S.fs[j] < S.fs[il]) il = j;
          if (S.fs[j] > S.fs[ih]) ih = j;
        }
        if (ih == il) ih = il == 0 ? 1 : 0;   // (all equal or NaN: any other vertex)
        int is = il;
        for (int j = 0; j <= S.k; ++j)
          if (j != ih && S.fs[j] > S.fs[is]) is = j;
        S.il = il; S.ih = ih; S.is = is;
        if (sbx_size(S, il) <= PSI * S.size0) { S.phase = P_END_SUB; break; }
        for (int d = 0; d < S.k; ++d) {
          double c = 0;
          for (int j = 0; j <= S.k; ++j)
            if (j != ih) c += S.simp[j][d];
          S.cen[d] = c / S.k;
          S.yr[d] = nl_clamp(S, S.perm[S.start + d], S.cen[d] + (S.cen[d] - S.simp[ih][d]));
        }
        if (!sbx_request(S, S.yr, P_REFL)) { sbx_take_best(S); S.phase = P_DONE; break; }
        return 1;
      }
      case P_REFL: {
        S.fr = fv;
        const int ih = S.ih;
        int next;
        if (S.fr < S.fs[S.il]) {
          for (int d = 0; d < S.k; ++d) S.y[d] = nl_clamp(S, S.perm[S.start + d], S.cen[d] + 2.0 * (S.cen[d] - S.simp[ih][d]));
          next = P_EXPD;
        } else if (S.fr < S.fs[S.is]) {
          for (int d = 0; d < S.k; ++d) S.simp[ih][d] = S.yr[d];
          S.fs[ih] = S.fr;
          S.phase = P_ITER;
          break;
        } else if (S.fr < S.fs[ih]) {
          for (int d = 0; d < S.k; ++d) S.y[d] = nl_clamp(S, S.perm[S.start + d], S.cen[d] + 0.5 * (S.yr[d] - S.cen[d]));
          next = P_CONT_OUT;
        } else {
          for (int d = 0; d < S.k; ++d) S.y[d] = nl_clamp(S, S.perm[S.start + d], S.cen[d] + 0.5 * (S.simp[ih][d] - S.cen[d]));
          next = P_CONT_IN;
        }
        if (!sbx_request(S, S.y, next)) { sbx_take_best(S); S.phase = P_DONE; break; }
        return 1;
      }
      case P_EXPD: {
        const bool e = fv < S.fr;
        for (int d = 0; d < S.k; ++d) S.simp[S.ih][d] = e ? S.y[d] : S.yr[d];
        S.fs[S.ih] = e ? fv : S.fr;
        S.phase = P_ITER;
        break;
      }
      case P_CONT_OUT:
      case P_CONT_IN:
        if (S.phase == P_CONT_OUT ? fv <= S.fr : fv < S.fs[S.ih]) {
          for (int d = 0; d < S.k; ++d) S.simp[S.ih][d] = S.y[d];
          S.fs[S.ih] = fv;
          S.phase = P_ITER;
        } else {
          S.jv = 0;
          S.phase = P_SHRINK_NEXT;
        }
        break;
      case P_SHRINK_GOT:
        for (int d = 0; d < S.k; ++d) S.simp[S.jv][d] = S.y[d];
        S.fs[S.jv] = fv;
        ++S.jv;
        S.phase = P_SHRINK_NEXT;
        // fall through
      case P_SHRINK_NEXT:
        if (S.jv == S.il) ++S.jv;
        if (S.jv > S.k) { S.phase = P_ITER; break; }
        for (int d = 0; d < S.k; ++d) S.y[d] = nl_clamp(S, S.perm[S.start + d], S.simp[S.il][d] + 0.5 * (S.simp[S.jv][d] - S.simp[S.il][d]));
        if (!sbx_request(S, S.y, P_SHRINK_GOT)) { sbx_take_best(S); S.phase = P_DONE; break; }
        return 1;
      case P_END_SUB:
        sbx_take_best(S);
        S.start += S.k;
        S.phase = ++S.isub < S.nsub ? P_SUB : P_END_CYCLE;
        break;
      case P_END_CYCLE: {
        bool moved = false;
        double ndx = 0, nst = 0;
        for (int i = 0; i < n; ++i) {
          S.dx[i] = S.x[i] - S.xprev[i];
          moved = moved || S.dx[i] != 0.0;
          ndx += fabs(S.dx[i]);
          nst += fabs(S.step[i]);
        }
        ++S.cycle;
        if (moved && S.fprev - S.f < S.frel * fabs(S.f)) { S.phase = P_DONE; break; }
        double sc = PSI;
        if (S.nsub > 1) {
          sc = ndx / nst;
          sc = sc < OMEGA ? OMEGA : (sc > 1.0 / OMEGA ? 1.0 / OMEGA : sc);
        }
        bool small = true;
        for (int i = 0; i < n; ++i) {
          const double a = fabs(S.step[i] * sc);
          S.step[i] = S.dx[i] > 0.0 ? a : (S.dx[i] < 0.0 ? -a : -(S.step[i] * sc));
          small = small && fabs(S.step[i]) <= S.xrel * fabs(S.x[i]);
        }
        S.phase = small ? P_DONE : P_CYCLE;
        break;
      }
      default:
        return 0;
    }
  }
}

}  // namespace mpcq_nl

// mpcq_replan.hpp — device minimum-snap generator and trajectory-slot install (mpcq_replan, mpcq_replace_trajectories).
// Included from mpcq_api.hip only; not templated on the engine precision (trajectories are float64 in every precision).
//
// The device restatement of csrc/minsnap.cpp's mpcq_minsnap_generate_order + mpcq_minsnap_sample, one wavefront per quadrotor:
//  * segment forms in closed form: A(T)^-1_ia = A(1)^-1_ia T^(r_a - i) and M(T)_ab = M(1)_ab T^(r_a + r_b - 2 order + 1) (r_a = a % 4,
//    the derivative a vertex condition fixes), the unit matrices once per workgroup in LDS -- no per-segment 8 x 8 elimination;
//  * the free vertex derivatives from one Gaussian elimination with partial pivoting (row per lane, pivot as a wave max) on the
//    <= 18 x 18 system the three axes share, three right-hand sides;
//  * sampled peak speed / acceleration at the host's sample points, Horner in the host's order, one wave max each;
//  * the host's bisection of the time scale, literally (wave-uniform control flow);
//  * sampling (one lane per row, the host's piece lookup, Horner order and 6-decimal rounding) straight into the engine's slot.
// Floating-point contraction is off in these functions: the host library is built with -ffp-contract=off and the bisection has to
// see the same function as the host.
#pragma once

namespace mpcq {
namespace replan {

constexpr int NC = 8, MAXV = 8, MAXS = MAXV - 1, MAXF = 3 * (MAXV - 2), RW = MAXF + 3;   // coefficients, vertices, segments, unknowns, row width
// result codes (include/mpcq.h MPCQ_REPLAN_*)
constexpr int DONE = 0, SKIPPED = 1, BAD_INPUT = -1, LIMITS = -3, TOO_LONG = -4;

// LDS of one workgroup (doubles)
struct Lds {
  double V[MAXV][3];        // vertices: start, waypoints
  double T0[MAXS], T[MAXS]; // estimated / scaled segment times
  double Tp[MAXS][15];      // T^k, k = -7..7
  double A1i[NC][NC];       // A(1)^-1
  double M1[NC][NC];        // M(1) of the order
  double R[MAXF][RW];       // free-derivative system | 3 right-hand sides (solution after the solve)
  double coef[MAXS][3][NC];
  double ends[MAXS];        // running sum of the durations (sampling)
  double last[16];          // last row of the slot (install)
  int first[MAXS + 1], steps[MAXS];   // sample points of `violation`: first sample index and interval count per segment
  int flag;
};

__device__ inline double ipow(double t, int k) {   // t^k for |k| <= 7
  double r = 1.0;
  const int a = k < 0 ? -k : k;
  for (int i = 0; i < a; ++i) r *= t;
  return k < 0 ? 1.0 / r : r;
}

// A(1)^-1 by the host's elimination (one lane), M(1) for `order` (lanes over (a, b)).
// Also the start of mpcq_replan_nonlinear: mpcq_minsnap_nl.hpp nl_unit_forms restates it operation for operation for the host library,
// and host / device bit parity depends on the two staying identical (tests/test_replan_nonlinear.py) -- change both together.
__device__ inline void unit_forms(Lds& S, int order) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x;
  if (lane == 0) {   // (in LDS: a pivot row index is not a compile-time constant, register arrays would go to scratch)
    double (*A)[RW] = S.R, (*I)[NC] = S.A1i;
    for (int r = 0; r < 4; ++r)
      for (int i = 0; i < NC; ++i) {
        double f = 1;
        for (int k = 0; k < r; ++k) f *= (i - k);
        A[r][i] = i == r ? f : 0.0;          // derivative r at t = 0
        A[4 + r][i] = i < r ? 0.0 : f;       // ... at t = 1
      }
    for (int i = 0; i < NC; ++i)
      for (int j = 0; j < NC; ++j) I[i][j] = i == j ? 1.0 : 0.0;
    for (int c = 0; c < NC; ++c) {
      int p = c;
      for (int r = c + 1; r < NC; ++r)
        if (fabs(A[r][c]) > fabs(A[p][c])) p = r;
      if (p != c)
        for (int k = 0; k < NC; ++k) { const double t = A[p][k]; A[p][k] = A[c][k]; A[c][k] = t; const double u = I[p][k]; I[p][k] = I[c][k]; I[c][k] = u; }
      const double inv = 1.0 / A[c][c];
      for (int r = c + 1; r < NC; ++r) {
        const double f = A[r][c] * inv;
        if (f == 0.0) continue;
        for (int k = c; k < NC; ++k) A[r][k] -= f * A[c][k];
        for (int k = 0; k < NC; ++k) I[r][k] -= f * I[c][k];
      }
    }
    for (int c = NC - 1; c >= 0; --c)
      for (int k = 0; k < NC; ++k) {
        double s = I[c][k];
        for (int j = c + 1; j < NC; ++j) s -= A[c][j] * I[j][k];
        I[c][k] = s / A[c][c];
      }
  }
  __syncthreads();
  {
    const int a = lane >> 3, b = lane & 7;
    auto fall = [&](int i) { double f = 1; for (int k = 0; k < order; ++k) f *= (i - k); return f; };
    double s = 0;
    for (int i = order; i < NC; ++i)
      for (int j = order; j < NC; ++j) s += S.A1i[i][a] * (fall(i) * fall(j) / (i + j - 2 * order + 1)) * S.A1i[j][b];
    S.M1[a][b] = s;
  }
  __syncthreads();
}

// pieces at the scaled times S.T: coefficients into S.coef; false if the system is singular (wave-uniform).
// Also the start of mpcq_replan_nonlinear: mpcq_minsnap_nl.hpp nl_linear_dfree restates the assembly, elimination and back substitution
// operation for operation for the host library -- change both together (bit parity: tests/test_replan_nonlinear.py).
__device__ inline bool solve_pieces(Lds& S, int n, int order) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x, ns = n - 1, nf = 3 * (n - 2);
  for (int it = lane; it < ns * 15; it += 64) {
    const int s = it / 15, k = it - s * 15 - 7;
    S.Tp[s][k + 7] = ipow(S.T[s], k);
  }
  if (lane == 0) {   // the host's sample points: max(2, ceil(T_s / 0.01)) intervals per segment
    S.first[0] = 0;
    for (int s = 0; s < ns; ++s) {
      const double q = ceil(S.T[s] / 0.01);
      S.steps[s] = q > 2.0 ? (int)q : 2;
      S.first[s + 1] = S.first[s] + S.steps[s] + 1;
    }
  }
  __syncthreads();
  auto free_idx = [&](int v, int r) { return (v == 0 || v == n - 1 || r == 0) ? -1 : 3 * (v - 1) + (r - 1); };
  auto M = [&](int s, int a, int b) { return S.M1[a][b] * S.Tp[s][(a & 3) + (b & 3) - 2 * order + 1 + 7]; };
  // assembly: R[fa][fb] summed over the segments in the host's order; right-hand sides from the fixed positions
  for (int it = lane; it < nf * nf; it += 64) {
    const int fa = it / nf, fb = it - fa * nf, va = fa / 3 + 1, ra = fa % 3 + 1, vb = fb / 3 + 1, rb = fb % 3 + 1;
    double acc = 0.0;
    const int s0 = (va > vb ? va : vb) - 1, s1 = va < vb ? va : vb;
    for (int s = s0; s <= s1; ++s)
      if (s >= 0 && s < ns) acc += M(s, (va - s) * 4 + ra, (vb - s) * 4 + rb);
    S.R[fa][fb] = acc;
  }
  for (int it = lane; it < nf * 3; it += 64) {
    const int fa = it / 3, ax = it - fa * 3, va = fa / 3 + 1, ra = fa % 3 + 1;
    double acc = 0.0;
    for (int s = va - 1; s <= va; ++s) {
      if (s < 0 || s >= ns) continue;
      const int a = (va - s) * 4 + ra;
      for (int b = 0; b < 2 * 4; ++b) {
        const int vb = s + b / 4, rb = b % 4;
        if (free_idx(vb, rb) >= 0) continue;
        acc -= M(s, a, b) * (rb == 0 ? S.V[vb][ax] : 0.0);
      }
    }
    S.R[fa][nf + ax] = acc;
  }
  __syncthreads();
  // elimination with partial pivoting: row r on lane r, pivot = the first row of largest magnitude (the host's choice)
  for (int c = 0; c < nf; ++c) {
    const double mag = (lane >= c && lane < nf) ? fabs(S.R[lane][c]) : -1.0;
    const double best = wave_max(mag);
    const int p = (int)wave_min((lane >= c && lane < nf && mag == best) ? (double)lane : 1e9);
    if (!(best > 0.0)) return false;   // (uniform: every lane holds the reduction)
    if (p != c)
      for (int k = lane; k < nf + 3; k += 64) { const double t = S.R[p][k]; S.R[p][k] = S.R[c][k]; S.R[c][k] = t; }
    __syncthreads();
    if (lane > c && lane < nf) {
      const double f = S.R[lane][c] * (1.0 / S.R[c][c]);
      if (f != 0.0) {
        for (int k = c; k < nf; ++k) S.R[lane][k] -= f * S.R[c][k];
        for (int k = 0; k < 3; ++k) S.R[lane][nf + k] -= f * S.R[c][nf + k];
      }
    }
    __syncthreads();
  }
  if (lane < 3 && nf > 0)   // back substitution, one right-hand side per lane (no cross-lane dependence)
    for (int c = nf - 1; c >= 0; --c) {
      double s = S.R[c][nf + lane];
      for (int j = c + 1; j < nf; ++j) s -= S.R[c][j] * S.R[j][nf + lane];
      S.R[c][nf + lane] = s / S.R[c][c];
    }
  __syncthreads();
  // coefficients c = A(T)^-1 d, lanes over (segment, axis, coefficient)
  for (int it = lane; it < ns * 3 * NC; it += 64) {
    const int s = it / (3 * NC), ax = (it / NC) % 3, i = it % NC;
    double c = 0;
    for (int a = 0; a < 2 * 4; ++a) {
      const int v = s + a / 4, r = a % 4, f = free_idx(v, r);
      const double d = f >= 0 ? S.R[f][nf + ax] : (r == 0 ? S.V[v][ax] : 0.0);
      c += S.A1i[i][a] * S.Tp[s][r - i + 7] * d;
    }
    S.coef[s][ax][i] = c;
  }
  __syncthreads();
  return true;
}

// max(sampled peak speed / v_max, peak acceleration / a_max) of the pieces in S.coef (the host's `limits`, dt 0.01)
__device__ inline double violation(Lds& S, int ns, double v_max, double a_max) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x;
  double vm = 0, am = 0;
  for (int j = lane; j < S.first[ns]; j += 64) {   // (S.first / S.steps: solve_pieces)
    int s = 0;
    while (j >= S.first[s + 1]) ++s;
    const int k = j - S.first[s];
    const double t = S.T[s] * k / S.steps[s];
    double v[3], a[3];
    for (int ax = 0; ax < 3; ++ax) {
      const double* c = S.coef[s][ax];
      double vv = 0, aa = 0;
      for (int i = NC - 1; i >= 1; --i) vv = vv * t + i * c[i];
      for (int i = NC - 1; i >= 2; --i) aa = aa * t + (double)i * (i - 1) * c[i];
      v[ax] = vv; a[ax] = aa;
    }
    const double sv = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), sa = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    vm = vm < sv ? sv : vm;
    am = am < sa ? sa : am;
  }
  vm = wave_max(vm); am = wave_max(am);
  const double x = vm / v_max, y = am / a_max;
  return x < y ? y : x;
}

// The install step both entry points end in: rows [0, len) of slot b are in place; pad [len, Tmax) with row len - 1, set the
// length, rewind the cursor, clear the finished flag.
__device__ inline void slot_commit(Lds& S, double* traj, int Tmax, int b, int len, int* lens, int* idx, int* finished) {
  const int lane = threadIdx.x;
  __syncthreads();   // (the rows written by the other lanes are visible to the workgroup)
  double* slot = traj + (size_t)b * Tmax * NX;
  if (lane < NX) S.last[lane] = slot[(size_t)(len - 1) * NX + lane];
  __syncthreads();
  const size_t pad = (size_t)(Tmax - len) * NX;
  for (size_t e = lane; e < pad; e += 64) slot[(size_t)len * NX + e] = S.last[e % NX];
  if (lane == 0) { lens[b] = len; idx[b] = 0; finished[b] = 0; }
}

__device__ inline bool finite3(const double* p) { return __builtin_isfinite(p[0]) && __builtin_isfinite(p[1]) && __builtin_isfinite(p[2]); }

// Vertices of quadrotor b into S.V: the start point p0 [3], then its n_wp waypoints wp_b [n_wp,3].  False if one is not finite
// (wave-uniform).  Starts with a barrier, so that a workgroup may plan one quadrotor after another in the same LDS.
__device__ inline bool load_vertices(Lds& S, const double* p0, const double* wp_b, int n_wp) {
  const int lane = threadIdx.x, n = n_wp + 1;
  __syncthreads();
  if (lane < n) {
    const double* p = lane == 0 ? p0 : wp_b + (size_t)(lane - 1) * 3;
    for (int k = 0; k < 3; ++k) S.V[lane][k] = p[k];
  }
  if (lane == 0) S.flag = 0;
  __syncthreads();
  if (lane < n && !finite3(S.V[lane])) S.flag = 1;
  __syncthreads();
  return S.flag == 0;
}

// Rows [0, rows) of slot b from the pieces in S.coef with the segment ends in S.ends (mpcq_minsnap_sample: one lane per row, the host's
// piece lookup, Horner order and 6-decimal rounding), then the install (slot_commit).
__device__ inline void sample_install(Lds& S, double* traj, int Tmax, int* lens, int* idx, int* finished, int b, int ns, int rows, double dt) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x;
  double* slot = traj + (size_t)b * Tmax * NX;
  for (int k = lane; k < rows; k += 64) {
    const double t = k * dt;
    int seg = 0;
    while (seg < ns - 1 && !(t < S.ends[seg])) ++seg;
    const double tl = t - (seg > 0 ? S.ends[seg - 1] : 0.0);
    double row[NX];
    for (int i = 0; i < NX; ++i) row[i] = 0.0;
    row[3] = 1.0;
    for (int a = 0; a < 3; ++a) {
      const double* c = S.coef[seg][a];
      double p = 0.0, v = 0.0;
      for (int i = 0; i < 8; ++i) p = p * tl + c[7 - i];
      for (int i = 0; i < 7; ++i) v = v * tl + (7 - i) * c[7 - i];
      row[a] = rint(p * 1e6) / 1e6;
      row[7 + a] = rint(v * 1e6) / 1e6;
    }
    for (int i = 0; i < NX; ++i) slot[(size_t)k * NX + i] = row[i];
  }
  slot_commit(S, traj, Tmax, b, rows, lens, idx, finished);
}

// The flight of one quadrotor, by the wavefront that calls it: planned through [p0, wp_b[0..n_wp)] and, on DONE, installed in slot b.
// Returns the MPCQ_REPLAN_* code (wave-uniform).  Shared by replan_kernel (a host call) and mission_kernel (mpcq_mission.hpp, behind a period).
__device__ inline int plan_linear(Lds& S, double* traj, int Tmax, int* lens, int* idx, int* finished, int b, const double* p0, const double* wp_b,
                                  int n_wp, double v_max, double a_max, int order, double dt) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x, n = n_wp + 1, ns = n_wp;
  if (!load_vertices(S, p0, wp_b, n_wp)) return BAD_INPUT;
  // segment-time estimate (mpcq_minsnap_estimate_times)
  if (lane < ns) {
    double d2 = 0;
    for (int k = 0; k < 3; ++k) d2 += (S.V[lane + 1][k] - S.V[lane][k]) * (S.V[lane + 1][k] - S.V[lane][k]);
    const double d = sqrt(d2), t = 2.0 * d / v_max * (1.0 + 6.5 * v_max / a_max * exp(-2.0 * d / v_max));
    S.T0[lane] = t > 1e-3 ? t : 1e-3;
  }
  unit_forms(S, order);   // (its barriers publish T0)
  auto viol = [&](double scale) {   // > 1: over a limit (the host's `violation`)
    if (lane < ns) S.T[lane] = S.T0[lane] * scale;
    __syncthreads();
    if (!solve_pieces(S, n, order)) return 1e30;
    return violation(S, ns, v_max, a_max);
  };
  // the host's bracket and bisection (mpcq_minsnap_generate_order), literally
  double lo = 0.05, hi = 1.0;
  bool ok = true;
  while (viol(hi) > 1.0) { hi *= 1.6; if (hi > 1e3) { ok = false; break; } }
  if (ok) {
    if (viol(lo) <= 1.0) hi = lo;
    else
      for (int it = 0; it < 40 && hi - lo > 1e-4 * hi; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (viol(mid) > 1.0) lo = mid; else hi = mid;
      }
    ok = viol(hi) <= 1.0;   // (leaves the pieces of `hi` in S.coef)
  }
  if (!ok) return LIMITS;
  // sampling (mpcq_minsnap_sample): durations T[s] = T0[s] hi
  double total = 0;
  for (int s = 0; s < ns; ++s) total = total + S.T[s];
  const int rows = (int)ceil(total / dt);
  if (rows > Tmax) return TOO_LONG;
  if (lane == 0) {
    double e = 0;
    for (int s = 0; s < ns; ++s) { e = e + S.T[s]; S.ends[s] = e; }
  }
  __syncthreads();
  sample_install(S, traj, Tmax, lens, idx, finished, b, ns, rows, dt);
  return DONE;
}

// One workgroup (one wavefront) per quadrotor.  start: [B,3] or the plant state [B,13] (start_stride 13); mask: [B] or NULL (the
// finished flags select).  code [B]: MPCQ_REPLAN_*.
__global__ __launch_bounds__(64) void replan_kernel(double* traj, int Tmax, int* lens, int* idx, int* finished, const double* start, int start_stride,
                                                    const double* wp, int n_wp, double v_max, double a_max, int order, double dt,
                                                    const int* mask, int* code) {
  Lds& S = *reinterpret_cast<Lds*>(smem_raw);
  const int b = blockIdx.x;
  const bool sel = mask ? mask[b] != 0 : finished[b] != 0;
  int c = SKIPPED;
  if (sel) c = plan_linear(S, traj, Tmax, lens, idx, finished, b, start + (size_t)b * start_stride, wp + (size_t)b * n_wp * 3, n_wp, v_max, a_max, order, dt);
  if (threadIdx.x == 0) code[b] = c;
}

// mpcq_replace_trajectories: host-made rows stage [count, Tmax, 13] into the slots sel[0..count)
__global__ __launch_bounds__(64) void install_kernel(double* traj, int Tmax, int* lens, int* idx, int* finished, const double* stage, const int* sel,
                                                     const int* len) {
  Lds& S = *reinterpret_cast<Lds*>(smem_raw);
  const int j = blockIdx.x, b = sel[j], n = len[j];
  const double* src = stage + (size_t)j * Tmax * NX;
  double* dst = traj + (size_t)b * Tmax * NX;
  for (size_t e = threadIdx.x; e < (size_t)n * NX; e += 64) dst[e] = src[e];
  slot_commit(S, traj, Tmax, b, n, lens, idx, finished);
}

}  // namespace replan
}  // namespace mpcq

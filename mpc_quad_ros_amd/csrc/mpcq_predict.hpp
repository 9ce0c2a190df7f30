// mpcq_predict.hpp — the RGP read-out (mpcq_rgp_predict / mpcq_record_predict): posterior mean and variance of every quadrotor's
// learned drag model at query points, evaluated on the device from the resident state or from a recording's buffers in place.
// Included from mpcq_api.hip only; the step kernel and its state are untouched.
//
// Per (quadrotor, axis, query point x), all in fp64 (src/gp/RGP.py:199-210; static GP: src/gp/GP.py:135-179, no C term):
//    k*_j = sf^2 exp(-(x - X_j)^2 / (2 L^2))      J = k* K_x^-1      mean = J mu      var = (sf^2 - J k*^T) + J C J^T
//
//  * predict_prep_kernel (shared grid only): J^T [3][nb][M] and b = sf^2 - J k*^T [3][M] depend on the axis alone and are built once
//    per call, one lane per query point, K_x^-1 of the axis in LDS.
//  * predict_kernel: one wavefront per (set, axis); a set is a quadrotor of the live state or a (quadrotor, row) of a recording
//    (pointer + strides for mu and C, so both entry points run the same code on the same numbers).  C and mu are read from global
//    memory once, coalesced, and staged in LDS as fp64 (nb <= STAGE_NB; larger models read C through the cache with wave-uniform
//    addresses).  Lanes run over the query points in tiles of 64; every lane keeps its own J column in LDS ([i][lane]: consecutive lanes,
//    consecutive words) and accumulates its own mean and quadratic form; the C and K_x^-1 operands are same-address LDS reads
//    (broadcast), four rows per pass so that a J word is read once per four multiply-adds.  Queries of their own per quadrotor
//    (per_quad) build J in this kernel with the routine the prep kernel uses.
// A lane reads only LDS words it wrote itself or that were staged in front of the one barrier: no barrier inside the tile loop.
// Every output is one sequential fused-multiply-add chain in ascending index order: independent of B, grouping and launch shape.
// Plain vector loads and stores, no atomics.
#pragma once

namespace mpcq {
namespace predict {

constexpr int MAX_M = 4096;     // query points per call
constexpr int STAGE_NB = 64;    // C (and K_x^-1) staged in LDS up to this basis size: 2 x 32 KiB + 2 x 32 KiB of columns at most

// LDS map in doubles (every part starts on a 16-byte boundary)
struct Lay { int C, K, mu, X, J, k, total; };
__host__ __device__ inline Lay layout(int nb, bool stage_C, bool build_J) {
  const int nn = (nb * nb + 1) & ~1, n1 = (nb + 1) & ~1;
  Lay L;
  int o = 0;
  L.C = o; o += stage_C ? nn : 0;
  L.K = o; o += build_J && nb <= STAGE_NB ? nn : 0;
  L.mu = o; o += n1;
  L.X = o; o += n1;
  L.J = o; o += 64 * nb;
  L.k = o; o += build_J ? 64 * nb : 0;
  L.total = o;
  return L;
}

template <typename TQ>
struct Args {
  const TQ* mu; const TQ* C;    // first set's mean [3][nb] and covariance [3][nb][nb]; C == nullptr: no J C J^T term (var not asked for, static GP)
  long mu_stride, C_stride;     // elements from one slab to the next
  const int* pos;               // recording: set s = (caller's quadrotor j, row k) = (s / nrows, s % nrows) reads slab (row0 + k) * count + pos[j];
  int row0, nrows, count;       //            nullptr: set s reads slab s
  const double* xq;             // per_quad: [nsets][3][M] (Jt == nullptr)
  const double* Jt; const double* bq;   // shared grid: what predict_prep_kernel wrote
  const double* Kinv; const double* basis;   // [3][nb][nb], [3][nb]
  double sf2[3], hl2[3];        // sigma_f^2 and 1 / (2 L^2) per axis
  double* mean; double* var;    // [nsets][3][M]; either may be nullptr
  int nb, M;
};

// a[r] = sum_j A[(i0 + r) nb + j] v[j][lane], r < R: R sequential chains over ascending j (A wave-uniform, v this lane's column)
template <int R, typename TA>
__device__ inline void rows_dot(const TA* A, int i0, int nb, const double* v, int lane, double* a) {
#pragma unroll
  for (int r = 0; r < R; ++r) a[r] = 0.0;
  for (int j = 0; j < nb; ++j) {
    const double vj = v[j * 64 + lane];
#pragma unroll
    for (int r = 0; r < R; ++r) a[r] = fma((double)A[(size_t)(i0 + r) * nb + j], vj, a[r]);
  }
}

// This lane's column of J = k* K_x^-1 for query point x into Jl[i][lane] (k* into kl[j][lane]); returns b = sf^2 - J k*^T.
// K_x^-1 is symmetric to the bit (spd_inverse mirrors it), so its rows serve as its columns.
__device__ inline double build_J(double x, const double* Xs, const double* Kinv, double sf2, double hl2, int nb, double* kl, double* Jl, int lane) {
  for (int j = 0; j < nb; ++j) {
    const double dl = x - Xs[j];
    kl[j * 64 + lane] = sf2 * exp(-(dl * dl) * hl2);
  }
  double a[4];
  int i = 0;
  for (; i + 4 <= nb; i += 4) {
    rows_dot<4>(Kinv, i, nb, kl, lane, a);
#pragma unroll
    for (int r = 0; r < 4; ++r) Jl[(i + r) * 64 + lane] = a[r];
  }
  for (; i < nb; ++i) {
    rows_dot<1>(Kinv, i, nb, kl, lane, a);
    Jl[i * 64 + lane] = a[0];
  }
  double s = 0.0;
  for (int j = 0; j < nb; ++j) s = fma(Jl[j * 64 + lane], kl[j * 64 + lane], s);
  return sf2 - s;
}

// J C J^T of this lane's column: sum over ascending i of J_i (C J^T)_i
template <typename TA>
__device__ inline double quad_form(const TA* C, int nb, const double* Jl, int lane) {
  double a[4], q = 0.0;
  int i = 0;
  for (; i + 4 <= nb; i += 4) {
    rows_dot<4>(C, i, nb, Jl, lane, a);
#pragma unroll
    for (int r = 0; r < 4; ++r) q = fma(Jl[(i + r) * 64 + lane], a[r], q);
  }
  for (; i < nb; ++i) {
    rows_dot<1>(C, i, nb, Jl, lane, a);
    q = fma(Jl[i * 64 + lane], a[0], q);
  }
  return q;
}

// K_x^-1 [nb][nb] and the basis [nb] of axis d for build_J: LDS copies up to STAGE_NB, the global arrays beyond
__device__ inline const double* stage_axis(const double* Kinv, const double* basis, int d, int nb, const Lay& L, double* sm, int lane) {
  for (int t = lane; t < nb; t += 64) sm[L.X + t] = basis[d * nb + t];
  const double* Kd = Kinv + (size_t)d * nb * nb;
  if (nb > STAGE_NB) return Kd;
  for (int t = lane; t < nb * nb; t += 64) sm[L.K + t] = Kd[t];
  return sm + L.K;
}

// grid: 3 x ceil(M / 64) workgroups of one wavefront; xq [3][M] -> Jt [3][nb][M], bq [3][M]
__global__ void __launch_bounds__(64) predict_prep_kernel(const double* xq, const double* Kinv, const double* basis, double sf2_0, double sf2_1, double sf2_2,
                                                          double hl2_0, double hl2_1, double hl2_2, int nb, int M, double* Jt, double* bq) {
  const int lane = threadIdx.x, tiles = (M + 63) / 64, d = blockIdx.x / tiles, m = (blockIdx.x - d * tiles) * 64 + lane;
  double* sm = reinterpret_cast<double*>(smem_raw);
  const Lay L = layout(nb, false, true);
  const double* Kl = stage_axis(Kinv, basis, d, nb, L, sm, lane);
  __syncthreads();
  const bool act = m < M;
  const double sf2 = d == 0 ? sf2_0 : (d == 1 ? sf2_1 : sf2_2), hl2 = d == 0 ? hl2_0 : (d == 1 ? hl2_1 : hl2_2);
  const double b = build_J(act ? xq[(size_t)d * M + m] : 0.0, sm + L.X, Kl, sf2, hl2, nb, sm + L.k, sm + L.J, lane);
  if (!act) return;
  for (int i = 0; i < nb; ++i) Jt[((size_t)d * nb + i) * M + m] = sm[L.J + i * 64 + lane];
  bq[(size_t)d * M + m] = b;
}

// grid: nsets x 3 workgroups of one wavefront.  STAGE: C in LDS (nb <= STAGE_NB)
template <typename TQ, bool STAGE>
__global__ void __launch_bounds__(64) predict_kernel(const Args<TQ> a) {
  const int lane = threadIdx.x, nb = a.nb, M = a.M;
  const size_t s = blockIdx.x / 3;
  const int d = (int)(blockIdx.x - s * 3);
  size_t slab = s;
  if (a.pos) {
    const int j = (int)(s / a.nrows), k = (int)(s - (size_t)j * a.nrows);
    slab = (size_t)(a.row0 + k) * a.count + a.pos[j];
  }
  const TQ* mu = a.mu + slab * a.mu_stride + (size_t)d * nb;
  const TQ* C = a.C ? a.C + slab * a.C_stride + (size_t)d * nb * nb : nullptr;
  const bool shared_grid = a.Jt != nullptr;
  double* sm = reinterpret_cast<double*>(smem_raw);
  const Lay L = layout(nb, STAGE && C, !shared_grid);
  for (int t = lane; t < nb; t += 64) sm[L.mu + t] = (double)mu[t];
  if (STAGE && C)
    for (int t = lane; t < nb * nb; t += 64) sm[L.C + t] = (double)C[t];
  const double* Kl = shared_grid ? nullptr : stage_axis(a.Kinv, a.basis, d, nb, L, sm, lane);
  __syncthreads();
  const double sf2 = d == 0 ? a.sf2[0] : (d == 1 ? a.sf2[1] : a.sf2[2]), hl2 = d == 0 ? a.hl2[0] : (d == 1 ? a.hl2[1] : a.hl2[2]);
  double* Jl = sm + L.J;
  const size_t o = (s * 3 + d) * (size_t)M;
  for (int m0 = 0; m0 < M; m0 += 64) {
    const int m = m0 + lane;
    const bool act = m < M;
    double b;
    if (shared_grid) {
      for (int i = 0; i < nb; ++i) Jl[i * 64 + lane] = act ? a.Jt[((size_t)d * nb + i) * M + m] : 0.0;
      b = act ? a.bq[(size_t)d * M + m] : 0.0;
    } else {
      b = build_J(act ? a.xq[o + m] : 0.0, sm + L.X, Kl, sf2, hl2, nb, sm + L.k, Jl, lane);
    }
    if (a.mean) {
      double mean = 0.0;
      for (int i = 0; i < nb; ++i) mean = fma(Jl[i * 64 + lane], sm[L.mu + i], mean);
      if (act) a.mean[o + m] = mean;
    }
    if (a.var) {
      double q = 0.0;
      if (C) q = STAGE ? quad_form(sm + L.C, nb, Jl, lane) : quad_form(C, nb, Jl, lane);
      if (act) a.var[o + m] = C ? b + q : b;
    }
  }
}

}  // namespace predict
}  // namespace mpcq

// mpcq_train.hpp — the device trainer (mpcq_rgp_train / mpcq_record_train): a drag model per (stream, axis) trained on all T samples
// of the stream in one persistent launch, from caller arrays or from a recording's MPCQ_RECORD_DRAG slab in place.
// Included from mpcq_api.hip only; the step kernel and its state are untouched.
//
// One 64-lane workgroup per regressor walks its samples in order; the regressor state stays in LDS from the first sample to the last
// and is written to global memory once at the end.  Two modes, both fp64:
//  * REGRESS = RGP.regress (src/gp/RGP.py:303-330) with fixed hyper-parameters, in the operation order of rgp_regress (mpcq_kernels.hpp):
//      k*_j = sf^2 exp(-(x - X_j)^2 / (2 L^2))   J = k* K_x^-1   G = C J^T / (sf^2 - J k*^T + J C J^T + sn^2)
//      mu += G (y - J mu)   C -= G (J C)          (not symmetrised, as in the reference)
//    start mu = 0, C = K(X,X) + sn^2 I; K_x^-1 is constant and staged once.
//  * LEARN = RGP.learn sample by sample: l_learn_sample of mpcq_learn_core.hpp, the routine mpcq_learn_step runs, from the start
//    values of learn_init_kernel (mu_g = 0, C_g = K_x, mu_eta = theta, C_eta = I, K_x^-1 by l_rebuild).
// Residency (template parameters RC, RK; chosen on the host, see train_run in mpcq_api.hip and DESIGN section 16): C and K_x^-1 live in
// LDS, or only C, or neither; a matrix that is not resident lives in its output array in global memory, as in learn_step_kernel.
// mu (and mu_eta, C_eta) are always resident.
// Samples are addressed by base pointer and strides: sample k of stream s, axis d is v[off(s) + k * step + d] with
// off(s) = (pos ? pos[s] : s) * stream_stride -- [S,T,3] caller arrays (stream_stride 3T, step 3) and the recorder's
// [capacity][count][6] slab (stream_stride 6, step 6 count, pos = place of the caller's quadrotor in the sorted selection) alike.
// Plain vector loads and stores, no atomics; every lane reads a sample through the same address.
#pragma once

#include "mpcq_learn_core.hpp"

namespace mpcq {
namespace train {

constexpr int REGRESS = 1, LEARN = 2;   // = MPCQ_TRAIN_REGRESS, MPCQ_TRAIN_LEARN (include/mpcq.h)
constexpr int MAX_NB = 64;

// LDS map in doubles
struct Lay { int C, K, mu, eta, X, scr, total; };
__host__ __device__ inline Lay layout(int nb, int mode, bool rc, bool rk) {
  const int nn = nb * nb;
  Lay L;
  int o = 0;
  L.C = o; o += rc ? nn : 0;
  L.K = o; o += rk ? nn : 0;
  L.mu = o; o += nb;
  L.eta = o; o += 12;          // LEARN: mu_eta [3] | C_eta [3][3]; REGRESS: the update's two scalars
  L.X = o; o += nb;
  L.scr = o; o += mode == LEARN ? (int)l_scratch_doubles((size_t)nb) : 4 * nb;   // REGRESS: ks Jt JC CJ [nb] each
  L.total = o;
  return L;
}

struct Args {
  int nb, T;                    // basis size, samples per stream
  const double* v; const double* a;   // inputs and targets of sample 0
  long stream_stride, step_stride;
  const int* pos;               // nullptr: stream s is slab s
  const double* basis;          // [3][nb]
  const double* theta;          // [3][3]
  const double* K0; const double* C0;   // REGRESS: K_x^-1 and K_x [3][nb][nb]
  double* mu; double* C;        // [R][nb], [R][nb][nb]            (R = 3 S regressors)
  double* mu_eta; double* C_eta; double* Kinv;   // LEARN: [R][3], [R][3][3], [R][nb][nb]
};

// grid: R workgroups of one wavefront
template <int MODE, bool RC, bool RK>
__global__ void __launch_bounds__(64) train_kernel(const Args a) {
  const int r = blockIdx.x, s = r / 3, d = r - 3 * s, n = a.nb, nn = n * n, t = threadIdx.x, NT = blockDim.x;
  double* sm = reinterpret_cast<double*>(smem_raw);
  const Lay L = layout(n, MODE, RC, RK);
  double* C = RC ? sm + L.C : a.C + (size_t)r * nn;
  double* mu = sm + L.mu;
  double* X = sm + L.X;
  double* D = sm + L.scr;
  const size_t off = (size_t)(a.pos ? a.pos[s] : s) * a.stream_stride + d;
  const double* vp = a.v + off;
  const double* ap = a.a + off;
  const double th0 = a.theta[d * 3], th1 = a.theta[d * 3 + 1], th2 = a.theta[d * 3 + 2];
  for (int j = t; j < n; j += NT) { X[j] = a.basis[d * n + j]; mu[j] = 0.0; }
  if (MODE == REGRESS) {
    const double* Kg = a.K0 + (size_t)d * nn;
    const double* K = RK ? sm + L.K : Kg;
    for (int i = t; i < nn; i += NT) C[i] = a.C0[(size_t)d * nn + i];
    if (RK)
      for (int i = t; i < nn; i += NT) sm[L.K + i] = Kg[i];
    double* ks = D;
    double* Jt = ks + n;
    double* JC = Jt + n;
    double* CJ = JC + n;
    double* sc = sm + L.eta;
    const double L2inv = 1.0 / (th0 * th0), sf2 = th1 * th1, sn2 = th2 * th2;
    double xt = vp[0], yt = ap[0];
    __syncthreads();
    for (int k = 0; k < a.T; ++k) {
      const double x = xt, y = yt;
      if (k + 1 < a.T) { xt = vp[(size_t)(k + 1) * a.step_stride]; yt = ap[(size_t)(k + 1) * a.step_stride]; }   // in flight during this sample
      for (int j = t; j < n; j += NT) {
        const double dl = x - X[j];
        ks[j] = sf2 * exp(-0.5 * dl * dl * L2inv);
      }
      __syncthreads();
      for (int j = t; j < n; j += NT) {
        double acc = 0;
        for (int i = 0; i < n; ++i) acc += ks[i] * K[i * n + j];
        Jt[j] = acc;
      }
      __syncthreads();
      for (int j = t; j < n; j += NT) {
        double p = 0, q = 0;
        for (int i = 0; i < n; ++i) { p += Jt[i] * C[i * n + j]; q += C[j * n + i] * Jt[i]; }
        JC[j] = p;
        CJ[j] = q;
      }
      __syncthreads();
      if (t == 0) {
        double mup = 0, Jk = 0, JCJ = 0;
        for (int i = 0; i < n; ++i) { mup += Jt[i] * mu[i]; Jk += Jt[i] * ks[i]; JCJ += JC[i] * Jt[i]; }
        const double Cp = sf2 - Jk + JCJ;
        sc[0] = y - mup;
        sc[1] = 1 / (Cp + sn2);
      }
      __syncthreads();
      for (int j = t; j < n; j += NT) mu[j] = mu[j] + CJ[j] * sc[1] * sc[0];
      for (int i = t; i < nn; i += NT) {
        const int row = i / n, col = i - row * n;
        C[i] = C[i] - CJ[row] * sc[1] * JC[col];
      }
      // (the next sample writes ks first and meets a barrier before anything written here is read or anything read here is written)
    }
    __syncthreads();
  } else {
    double* K = RK ? sm + L.K : a.Kinv + (size_t)r * nn;
    double* eta = sm + L.eta;
    double* Ce = eta + 3;
    __syncthreads();   // X
    for (int i = t; i < nn; i += NT) {
      const int row = i / n, col = i - row * n;
      C[i] = l_rbf(X[row], X[col], th0, th1) + (row == col ? th2 * th2 : 0.0);   // C_0 = K(X,X) + sigma_n^2 I
    }
    if (t < 3) eta[t] = a.theta[d * 3 + t];
    if (t < 9) Ce[t] = (t % 4 == 0) ? 1.0 : 0.0;
    l_rebuild(X, n, th0, th1, th2, D, D + nn, K, reinterpret_cast<int*>(D + 2 * nn));
    double xt = vp[0], yt = ap[0];
    __syncthreads();
    for (int k = 0; k < a.T; ++k) {
      const double x = xt, y = yt;
      if (k + 1 < a.T) { xt = vp[(size_t)(k + 1) * a.step_stride]; yt = ap[(size_t)(k + 1) * a.step_stride]; }
      l_learn_sample(X, n, mu, C, eta, Ce, K, x, y, D);
    }
    __syncthreads();
    if (t < 3) a.mu_eta[(size_t)r * 3 + t] = eta[t];
    if (t < 9) a.C_eta[(size_t)r * 9 + t] = Ce[t];
    if (RK)
      for (int i = t; i < nn; i += NT) a.Kinv[(size_t)r * nn + i] = K[i];
  }
  for (int j = t; j < n; j += NT) a.mu[(size_t)r * n + j] = mu[j];
  if (RC)
    for (int i = t; i < nn; i += NT) a.C[(size_t)r * nn + i] = C[i];
}

}  // namespace train
}  // namespace mpcq

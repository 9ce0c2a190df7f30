// mpcq_learn_core.hpp — the per-sample body of RGP.learn (src/gp/RGP.py:332-505) and the K_x^-1 rebuild, shared by the stepwise learner
// (mpcq_learn.hip: one sample per launch, state in global memory) and the device trainer (mpcq_train.hpp: all samples of a stream in
// one launch, state in LDS as far as it fits).  The routines take plain pointers for the regressor state; where a pointer leads --
// global memory or LDS -- is the caller's choice and changes no operation and no operation order.  One 64-lane workgroup per regressor.
#pragma once

namespace mpcq {

__device__ inline double l_rbf(double x1, double x2, double L, double sf) {
  const double d = x1 - x2, invLL = 1.0 / (L * L);
  return sf * sf * exp(((-0.5 * d) * invLL) * d);
}

// principal square root of a symmetric positive definite 3x3 matrix (scipy.linalg.sqrtm in the reference): Jacobi rotations
__device__ inline void l_sqrtm3(const double* A, double* S) {
  double a[9], v[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  for (int k = 0; k < 9; ++k) a[k] = A[k];
  for (int sweep = 0; sweep < 60; ++sweep) {
    const double off = a[1] * a[1] + a[2] * a[2] + a[5] * a[5];
    if (off < 1e-300) break;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        if (a[p * 3 + q] == 0.0) continue;
        const double th = (a[q * 3 + q] - a[p * 3 + p]) / (2 * a[p * 3 + q]);
        const double t = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1));
        const double c = 1 / sqrt(t * t + 1), sn = t * c;
        for (int k = 0; k < 3; ++k) { const double x = a[k * 3 + p], y = a[k * 3 + q]; a[k * 3 + p] = c * x - sn * y; a[k * 3 + q] = sn * x + c * y; }
        for (int k = 0; k < 3; ++k) { const double x = a[p * 3 + k], y = a[q * 3 + k]; a[p * 3 + k] = c * x - sn * y; a[q * 3 + k] = sn * x + c * y; }
        for (int k = 0; k < 3; ++k) { const double x = v[k * 3 + p], y = v[k * 3 + q]; v[k * 3 + p] = c * x - sn * y; v[k * 3 + q] = sn * x + c * y; }
      }
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double t = 0;
      for (int k = 0; k < 3; ++k) t += v[i * 3 + k] * sqrt(a[k * 3 + k]) * v[j * 3 + k];
      S[i * 3 + j] = t;
    }
}

// K_x = K(X,X) + sigma_n^2 I and its inverse into gout (global memory or LDS); M, Ai: LDS [n][n] each; one lane per row
__device__ inline void l_rebuild(const double* X, int n, double L, double sf, double sn, double* M, double* Ai, double* gout, int* piv) {
  const int t = threadIdx.x;
  for (int it = t; it < n * n; it += blockDim.x) {
    const int i = it / n, j = it - i * n;
    M[it] = l_rbf(X[i], X[j], L, sf) + (i == j ? sn * sn : 0.0);
    Ai[it] = i == j ? 1.0 : 0.0;
  }
  __syncthreads();
  for (int c = 0; c < n; ++c) {
    if (t == 0) {
      int p = c;
      for (int i = c + 1; i < n; ++i)
        if (fabs(M[i * n + c]) > fabs(M[p * n + c])) p = i;
      *piv = p;
    }
    __syncthreads();
    const int p = *piv;
    if (p != c && t < n) {
      const double a = M[p * n + t], b = M[c * n + t], ai = Ai[p * n + t], bi = Ai[c * n + t];
      M[p * n + t] = b; M[c * n + t] = a; Ai[p * n + t] = bi; Ai[c * n + t] = ai;
    }
    __syncthreads();
    const double d = 1.0 / M[c * n + c];
    __syncthreads();
    if (t < n) { M[c * n + t] *= d; Ai[c * n + t] *= d; }
    __syncthreads();
    if (t < n && t != c) {
      const double f = M[t * n + c];
      if (f != 0.0)
        for (int j = 0; j < n; ++j) { M[t * n + j] -= f * M[c * n + j]; Ai[t * n + j] -= f * Ai[c * n + j]; }
    }
    __syncthreads();
  }
  for (int it = t; it < n * n; it += blockDim.x) gout[it] = Ai[it];
}

// doubles of LDS scratch l_learn_sample needs at basis size n (the K_x^-1 rebuild of learn_init_kernel fits in it as well):
// Cp [np][np] | W [max(7 np, 2 n n)] | ks Jt CJ JC mug [n] each | Lt [n+2][2] | sc [32] | piv (one int in a double's place, +1 spare)
__host__ __device__ inline size_t l_scratch_doubles(size_t n) {
  const size_t np_ = n + 4, wsz = 7 * np_ > 2 * n * n ? 7 * np_ : 2 * n * n;
  return np_ * np_ + wsz + 5 * n + 2 * (n + 2) + 32 + 2;
}

// One sample (xt, yt) of RGP.learn for one regressor: updates mu_g [n], C_g [n][n], mu_eta [3], C_eta [3][3] and rebuilds K_x^-1 [n][n]
// for the new hyper-parameters.  X: the axis' basis [n]; D: LDS scratch of l_scratch_doubles(n).  Called by all lanes of the workgroup;
// the caller places a barrier between its own writes of the state and the call.  What a lane wrote of the state is visible to the
// other lanes behind the barriers of the K_x^-1 rebuild at the end, so calls may follow each other directly.
__device__ inline void l_learn_sample(const double* X, const int n, double* gmu, double* gC, double* geta, double* gCe, double* gKi,
                                      const double xt, const double yt, double* D) {
  const int t = threadIdx.x, NT = blockDim.x;
  const int np_ = n + 4, nu = n + 2, nz = n + 3;
  // LDS: Cp [np][np] | W [max(7 np, 2 n n)] (running means, later the Gauss-Jordan workspace) | ks Jt CJ JC mug [n] each | Lt [nu][2] | sc [32]
  double* Cp = D;
  double* W = Cp + np_ * np_;
  const int wsz = 7 * np_ > 2 * n * n ? 7 * np_ : 2 * n * n;
  double* ks = W + wsz;
  double* Jt = ks + n;
  double* CJ = Jt + n;
  double* JC = CJ + n;
  double* mug = JC + n;
  double* Lt = mug + n;
  double* sc = Lt + 2 * nu;
  int* piv = reinterpret_cast<int*>(sc + 32);
  const double e0 = geta[0], e1 = geta[1], e2 = geta[2];
  for (int j = t; j < n; j += NT) { ks[j] = l_rbf(xt, X[j], e0, e1); mug[j] = gmu[j]; }
  __syncthreads();
  for (int j = t; j < n; j += NT) { double a = 0; for (int i = 0; i < n; ++i) a += ks[i] * gKi[i * n + j]; Jt[j] = a; }
  __syncthreads();
  for (int i = t; i < n; i += NT) {
    double a = 0, b = 0;
    for (int j = 0; j < n; ++j) { a += gC[i * n + j] * Jt[j]; b += Jt[j] * gC[j * n + i]; }
    CJ[i] = a; JC[i] = b;
  }
  __syncthreads();
  if (t == 0) {
    double Jk = 0, JCJ = 0, Jmu = 0;
    for (int j = 0; j < n; ++j) { Jk += Jt[j] * ks[j]; JCJ += JC[j] * Jt[j]; Jmu += Jt[j] * mug[j]; }
    sc[0] = l_rbf(xt, xt, e0, e1) - Jk;   // B
    sc[1] = JCJ; sc[2] = Jmu;
    // sigma points: eta_hat[i][k] in sc[4 + 3 i + k]
    double C6[9], Sq[9];
    for (int k = 0; k < 9; ++k) C6[k] = 3.0 / (1 - 0.5) * gCe[k];
    l_sqrtm3(C6, Sq);
    const double mu[3] = {e0, e1, e2};
    for (int k = 0; k < 3; ++k) sc[4 + k] = mu[k];
    for (int i = 0; i < 3; ++i)
      for (int k = 0; k < 3; ++k) { sc[4 + 3 * (i + 1) + k] = mu[k] + Sq[k * 3 + i]; sc[4 + 3 * (i + 4) + k] = mu[k] - Sq[k * 3 + i]; }
  }
  __syncthreads();
  const double Bv = sc[0], JCJ = sc[1], Jmu = sc[2];
  auto w_of = [](int i) { return i == 0 ? 0.5 : (1 - 0.5) / 6.0; };
  auto mpi = [&](int i, int a) { return a < n ? mug[a] : (a < n + 3 ? sc[4 + 3 * i + (a - n)] : Jmu); };
  auto cpi = [&](int a, int b) {
    if (a < n && b < n) return gC[a * n + b];
    if (a < n && b == n + 3) return CJ[a];
    if (a == n + 3 && b < n) return JC[b];
    if (a == n + 3 && b == n + 3) return JCJ + Bv;
    return 0.0;
  };
  // running means mu_run[i][a] (the reference subtracts the mean accumulated SO FAR inside the loop)
  for (int a = t; a < np_; a += NT) {
    double m = 0;
    for (int i = 0; i < 7; ++i) { m += w_of(i) * mpi(i, a); W[i * np_ + a] = m; }
  }
  __syncthreads();
  for (int it = t; it < np_ * np_; it += NT) {
    const int a = it / np_, b = it - a * np_;
    const double c = cpi(a, b);
    double acc = 0;
    for (int i = 0; i < 7; ++i) acc += w_of(i) * ((mpi(i, a) - W[i * np_ + a]) * (mpi(i, b) - W[i * np_ + b]) + c);
    Cp[it] = acc;
  }
  __syncthreads();
  // observable o = [sigma_n, g_t] = rows nu, nu+1; every lane forms the 2x2 quantities itself
  const double mo0 = W[6 * np_ + nu], mo1 = W[6 * np_ + nu + 1];
  const double Co00 = Cp[nu * np_ + nu], Co01 = Cp[nu * np_ + nu + 1], Co10 = Cp[(nu + 1) * np_ + nu], Co11 = Cp[(nu + 1) * np_ + nu + 1];
  const double Cy = Co11 + Co00 + mo0 * mo0;
  const double G0 = Co01 / Cy, G1 = Co11 / Cy;
  const double me0 = mo0 + G0 * (yt - mo1), me1 = mo1 + G1 * (yt - mo1);
  const double Ce00 = Co00 - G0 * Cy * G0, Ce01 = Co01 - G0 * Cy * G1, Ce10 = Co10 - G1 * Cy * G0, Ce11 = Co11 - G1 * Cy * G1;
  const double det = Co00 * Co11 - Co01 * Co10;
  const double Ci00 = Co11 / det, Ci01 = -Co01 / det, Ci10 = -Co10 / det, Ci11 = Co00 / det;
  for (int a = t; a < nu; a += NT) {
    const double c0 = Cp[nu * np_ + a], c1 = Cp[(nu + 1) * np_ + a];
    Lt[a * 2] = c0 * Ci00 + c1 * Ci10;
    Lt[a * 2 + 1] = c0 * Ci01 + c1 * Ci11;
  }
  __syncthreads();
  const double D00 = Ce00 - Co00, D01 = Ce01 - Co01, D10 = Ce10 - Co10, D11 = Ce11 - Co11;
  auto mu_z = [&](int a) { return a < nu ? W[6 * np_ + a] + Lt[a * 2] * (me0 - mo0) + Lt[a * 2 + 1] * (me1 - mo1) : me0; };
  auto C_z = [&](int a, int b) {
    if (a < nu && b < nu) {
      const double t0 = Lt[a * 2] * D00 + Lt[a * 2 + 1] * D10, t1 = Lt[a * 2] * D01 + Lt[a * 2 + 1] * D11;
      return Cp[a * np_ + b] + t0 * Lt[b * 2] + t1 * Lt[b * 2 + 1];
    }
    if (a < nu) return Lt[a * 2] * Ce00 + Lt[a * 2 + 1] * Ce10;
    if (b < nu) return Ce00 * Lt[b * 2] + Ce01 * Lt[b * 2 + 1];
    return Ce00;
  };
  (void)nz;
  for (int a = t; a < n; a += NT) gmu[a] = mu_z(a);
  for (int it = t; it < n * n; it += NT) { const int a = it / n, b = it - a * n; gC[it] = C_z(a, b); }
  double ne[3];
  for (int a = 0; a < 3; ++a) ne[a] = mu_z(n + a);
  if (t < 3) geta[t] = ne[t];
  if (t < 9) gCe[t] = C_z(n + t / 3, n + t % 3);
  __syncthreads();   // W (running means) is read above; it becomes the Gauss-Jordan workspace now
  l_rebuild(X, n, ne[0], ne[1], ne[2], W, W + n * n, gKi, piv);
}

}  // namespace mpcq

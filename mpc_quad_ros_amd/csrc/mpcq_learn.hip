// mpcq_learn.hip — batched RGP.learn (src/gp/RGP.py:332-505): hyper-parameter learning of the recursive GP for B x 3
// independent (quadrotor, axis) regressors, one 64-lane workgroup per regressor, fp64, state resident in HBM.
// SURVEY §8 f4 ("next" row): the loop body of the node never calls learn (it is the reference's offline estimator), so this
// is its own small object behind the C ABI (mpcq_learn_* in include/mpcq.h), not part of the fused control step.
//
// What one call does per regressor with the new scalar sample (s, y), in the reference's operation order:
//   Jt = k(s, X) K_x^-1, B = k(s,s) - Jt k(X,s)                                   (gain at the CURRENT hyper-parameters)
//   sigma points of eta = (L, sigma_f, sigma_n): eta_0 = mu, eta_i = mu +- sqrtm(6 C_eta)[:, i], w = (1/2, 1/12 ...)
//   p = [g, eta, g_t]: mu_p, C_p accumulated over the 7 points WITH THE RUNNING MEAN inside the loop (as the reference)
//   Kalman update of the observable part o = [sigma_n, g_t] with C_y = C_o[1,1] + C_o[0,0] + mu_o[0]^2, smoother-type
//   update of the rest u = [g, L, sigma_f] through Lt = C_ou' C_o^-1; new (mu_g, C_g, mu_eta, C_eta)
//   K_x = K(X,X) + sigma_n^2 I and K_x^-1 (Gauss-Jordan with partial pivoting) for the new hyper-parameters.
// The cross-covariance C_g_eta of the reference is never updated there (it stays zero), so the St terms vanish.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mpcq.h"
#include "mpcq_learn_core.hpp"   // l_rbf, l_sqrtm3, l_rebuild, l_learn_sample

namespace mpcq {
extern __shared__ unsigned char smem_raw[];

struct LearnState {
  int B, n;
  const double* X;     // [3][n] basis vectors (shared by the batch)
  double* mu_g;        // [B][3][n]
  double* C_g;         // [B][3][n][n]
  double* mu_eta;      // [B][3][3]
  double* C_eta;       // [B][3][3][3]
  double* Kxinv;       // [B][3][n][n]
};

__global__ void __launch_bounds__(64) learn_init_kernel(const LearnState st, const double* theta /*[3][3]*/) {
  const int r = blockIdx.x, d = r % 3, n = st.n, t = threadIdx.x;
  double* D = reinterpret_cast<double*>(smem_raw);
  double* M = D;
  double* Ai = D + n * n;
  int* piv = reinterpret_cast<int*>(D + 2 * n * n);
  const double* X = st.X + d * n;
  const double L = theta[d * 3], sf = theta[d * 3 + 1], sn = theta[d * 3 + 2];
  for (int it = t; it < n; it += blockDim.x) st.mu_g[(size_t)r * n + it] = 0.0;
  for (int it = t; it < n * n; it += blockDim.x) {
    const int i = it / n, j = it - i * n;
    st.C_g[(size_t)r * n * n + it] = l_rbf(X[i], X[j], L, sf) + (i == j ? sn * sn : 0.0);   // C_0 = K(X,X) + sigma_n^2 I
  }
  if (t < 3) st.mu_eta[(size_t)r * 3 + t] = theta[d * 3 + t];
  if (t < 9) st.C_eta[(size_t)r * 9 + t] = (t % 4 == 0) ? 1.0 : 0.0;
  l_rebuild(X, n, L, sf, sn, M, Ai, st.Kxinv + (size_t)r * n * n, piv);
}

__global__ void __launch_bounds__(64) learn_step_kernel(const LearnState st, const double* s_in, const double* y_in) {
  const int r = blockIdx.x, d = r % 3, n = st.n;
  l_learn_sample(st.X + d * n, n, st.mu_g + (size_t)r * n, st.C_g + (size_t)r * n * n, st.mu_eta + (size_t)r * 3, st.C_eta + (size_t)r * 9,
                 st.Kxinv + (size_t)r * n * n, s_in[r], y_in[r], reinterpret_cast<double*>(smem_raw));
}

}  // namespace mpcq

// ------------------------------------------------------------------ C ABI
namespace {
thread_local std::string l_err;
int lfail(int code, const std::string& msg) { l_err = msg; return code; }
#define L_TRY(expr)                                                                                  \
  do {                                                                                               \
    hipError_t _e = (expr);                                                                          \
    if (_e != hipSuccess) return lfail(MPCQ_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)
struct Guard {
  int prev = -1; bool sw = false;
  explicit Guard(int dev) { if (hipGetDevice(&prev) == hipSuccess && prev != dev) sw = hipSetDevice(dev) == hipSuccess; }
  ~Guard() { if (sw) (void)hipSetDevice(prev); }
};
}  // namespace

struct mpcq_learner {
  mpcq::LearnState st;
  int device = 0;
  size_t lds = 0;
  hipStream_t stream = nullptr;
  double *d_X = nullptr, *d_theta = nullptr, *d_s = nullptr, *d_y = nullptr;
};

extern "C" {

const char* mpcq_learn_last_error(void) { return l_err.c_str(); }

int mpcq_learn_create(int32_t batch, int32_t nb, const double* basis, const double* theta, int32_t device, mpcq_learner** out) {
  if (!out) return lfail(MPCQ_ERR_INVALID, "null argument");
  *out = nullptr;
  if (batch <= 0 || nb < 1 || nb > 64 || !basis || !theta) return lfail(MPCQ_ERR_INVALID, "bad batch / nb (1..64) / basis / theta");
  for (int d = 0; d < 3; ++d)
    if (!(theta[d * 3] > 0)) return lfail(MPCQ_ERR_INVALID, "theta: length scale must be > 0");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return lfail(MPCQ_ERR_DEVICE, "no HIP device: libmpcq has no CPU path");
  if (device < 0 || device >= ndev) return lfail(MPCQ_ERR_INVALID, "device ordinal out of range");
  Guard g(device);
  mpcq_learner* l = new mpcq_learner();
  l->device = device;
  const size_t R = (size_t)batch * 3, n = nb;
  std::memset(&l->st, 0, sizeof(l->st));
  l->st.B = batch; l->st.n = nb;
  auto fail_free = [&](int rc) { mpcq_learn_destroy(l); return rc; };
#define L_ALLOC(p, cnt) if (hipMalloc((void**)&(p), (cnt) * sizeof(double)) != hipSuccess) return fail_free(lfail(MPCQ_ERR_DEVICE, "hipMalloc"))
  L_ALLOC(l->d_X, 3 * n); L_ALLOC(l->d_theta, 9); L_ALLOC(l->d_s, R); L_ALLOC(l->d_y, R);
  L_ALLOC(l->st.mu_g, R * n); L_ALLOC(l->st.C_g, R * n * n); L_ALLOC(l->st.mu_eta, R * 3); L_ALLOC(l->st.C_eta, R * 9); L_ALLOC(l->st.Kxinv, R * n * n);
#undef L_ALLOC
  l->st.X = l->d_X;
  if (hipStreamCreateWithFlags(&l->stream, hipStreamNonBlocking) != hipSuccess) return fail_free(lfail(MPCQ_ERR_DEVICE, "hipStreamCreate"));
  l->lds = mpcq::l_scratch_doubles(n) * sizeof(double);
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&mpcq::learn_step_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)l->lds) != hipSuccess ||
      hipFuncSetAttribute(reinterpret_cast<const void*>(&mpcq::learn_init_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)l->lds) != hipSuccess)
    return fail_free(lfail(MPCQ_ERR_DEVICE, "hipFuncSetAttribute"));
  if (hipMemcpyAsync(l->d_X, basis, 3 * n * sizeof(double), hipMemcpyHostToDevice, l->stream) != hipSuccess ||
      hipMemcpyAsync(l->d_theta, theta, 9 * sizeof(double), hipMemcpyHostToDevice, l->stream) != hipSuccess)
    return fail_free(lfail(MPCQ_ERR_DEVICE, "hipMemcpy"));
  hipLaunchKernelGGL(mpcq::learn_init_kernel, dim3((unsigned)R), dim3(64), l->lds, l->stream, l->st, l->d_theta);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(l->stream) != hipSuccess) return fail_free(lfail(MPCQ_ERR_DEVICE, "learn_init_kernel"));
  *out = l;
  return 0;
}

int mpcq_learn_destroy(mpcq_learner* l) {
  if (!l) return 0;
  Guard g(l->device);
  void* ptrs[] = {l->d_X, l->d_theta, l->d_s, l->d_y, l->st.mu_g, l->st.C_g, l->st.mu_eta, l->st.C_eta, l->st.Kxinv};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  if (l->stream) (void)hipStreamDestroy(l->stream);
  delete l;
  return 0;
}

int mpcq_learn_step(mpcq_learner* l, const double* v_body, const double* a_drag) {
  if (!l || !v_body || !a_drag) return lfail(MPCQ_ERR_INVALID, "null argument");
  Guard g(l->device);
  const size_t R = (size_t)l->st.B * 3;
  L_TRY(hipMemcpyAsync(l->d_s, v_body, R * sizeof(double), hipMemcpyHostToDevice, l->stream));
  L_TRY(hipMemcpyAsync(l->d_y, a_drag, R * sizeof(double), hipMemcpyHostToDevice, l->stream));
  hipLaunchKernelGGL(mpcq::learn_step_kernel, dim3((unsigned)R), dim3(64), l->lds, l->stream, l->st, l->d_s, l->d_y);
  L_TRY(hipGetLastError());
  L_TRY(hipStreamSynchronize(l->stream));
  return 0;
}

int mpcq_learn_get(mpcq_learner* l, double* mu_g, double* C_g, double* mu_eta, double* C_eta, double* Kx_inv) {
  if (!l) return lfail(MPCQ_ERR_INVALID, "null argument");
  Guard g(l->device);
  const size_t R = (size_t)l->st.B * 3, n = l->st.n;
  if (mu_g) L_TRY(hipMemcpyAsync(mu_g, l->st.mu_g, R * n * sizeof(double), hipMemcpyDeviceToHost, l->stream));
  if (C_g) L_TRY(hipMemcpyAsync(C_g, l->st.C_g, R * n * n * sizeof(double), hipMemcpyDeviceToHost, l->stream));
  if (mu_eta) L_TRY(hipMemcpyAsync(mu_eta, l->st.mu_eta, R * 3 * sizeof(double), hipMemcpyDeviceToHost, l->stream));
  if (C_eta) L_TRY(hipMemcpyAsync(C_eta, l->st.C_eta, R * 9 * sizeof(double), hipMemcpyDeviceToHost, l->stream));
  if (Kx_inv) L_TRY(hipMemcpyAsync(Kx_inv, l->st.Kxinv, R * n * n * sizeof(double), hipMemcpyDeviceToHost, l->stream));
  L_TRY(hipStreamSynchronize(l->stream));
  return 0;
}

}  // extern "C"

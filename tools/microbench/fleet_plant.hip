// Measurement (GPU box): device time of fleet_plant_kernel (mpcq_fleet.hpp: every quadrotor its own plant) next to plant_kernel
// (mpcq_kernels.hpp: the engine's shared plant), the kernel whose place it takes in a period.  Both are launched as the engine launches
// them -- one lane per quadrotor, blocks of 64 -- alternately in one process, each launch between a HIP-event pair of its own, from the
// same start states (restored in front of every launch, outside the pair) and with the same controls.  Default plants, so that both
// kernels integrate the same flight.  Prints one JSON object per batch size.
//   build: hipcc -O2 --offload-arch=gfx950 -std=c++17 -fno-strict-aliasing -o fleet_plant fleet_plant.hip
//   run:   ./fleet_plant [n_sub sim_dt launches B ...]     (defaults: 2 5e-3 200 1024 8192: the plant update of the bench workload)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/mpcq.h"
#include "../../mpc_quad_ros_amd/csrc/mpcq_kernels.hpp"
#include "../../mpc_quad_ros_amd/csrc/mpcq_fleet.hpp"

#define CHECK(expr)                                                                                  \
  do {                                                                                               \
    hipError_t e_ = (expr);                                                                          \
    if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e_)); return 1; } \
  } while (0)

static double median(std::vector<float> v) {
  std::sort(v.begin(), v.end());
  return 0.5 * (v[(v.size() - 1) / 2] + v[v.size() / 2]);
}

int main(int argc, char** argv) {
  const int n_sub = argc > 1 ? std::atoi(argv[1]) : 2;
  const double sim_dt = argc > 2 ? std::atof(argv[2]) : 5e-3;
  const int launches = argc > 3 ? std::atoi(argv[3]) : 200, warm = 20;
  std::vector<int> batches;
  for (int i = 4; i < argc; ++i) batches.push_back(std::atoi(argv[i]));
  if (batches.empty()) batches = {1024, 8192};
  if (n_sub < 1 || !(sim_dt > 0) || launches < 1) { std::fprintf(stderr, "bad arguments\n"); return 1; }
  // the hummingbird of mpc_quad_ros_amd/params.py
  mpcq::DevModel<double> m;
  std::memset(&m, 0, sizeof(m));
  const double L = 0.17, c = 0.016;
  m.mass = 0.68 + 4 * 0.009; m.imass = 1.0 / m.mass; m.tmax = 838.0 * 838.0 * 8.54858e-06; m.g = 9.81; m.aero_drag = 0.008;
  const double J[3] = {0.007, 0.007, 0.012}, rd[3] = {0.3, 0.3, 0.0}, xf[4] = {L, 0, -L, 0}, yf[4] = {0, L, 0, -L}, zl[4] = {c, -c, c, -c};
  mpcq_plant p;
  std::memset(&p, 0, sizeof(p));
  p.mass = m.mass; p.max_thrust = m.tmax; p.aero_drag = m.aero_drag;
  for (int i = 0; i < 3; ++i) { m.J[i] = p.J[i] = J[i]; m.iJ[i] = 1.0 / J[i]; m.rotor_drag[i] = p.rotor_drag[i] = rd[i]; }
  for (int j = 0; j < 4; ++j) { m.xf[j] = p.x_f[j] = xf[j]; m.yf[j] = p.y_f[j] = yf[j]; m.zl[j] = p.z_l_tau[j] = zl[j]; p.rotor_functionality[j] = 1.0; }
  hipStream_t s;
  hipEvent_t e0, e1;
  CHECK(hipStreamCreate(&s));
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  for (const int B : batches) {
    if (B < 1) { std::fprintf(stderr, "bad batch\n"); return 1; }
    std::vector<double> x0((size_t)B * 13, 0.0), w((size_t)B * 4), tab((size_t)mpcq::fleet::NF * B), row(mpcq::fleet::NF), xa((size_t)B * 13), xb((size_t)B * 13);
    unsigned r = 12345u;
    auto uni = [&r]() { r = r * 1664525u + 1013904223u; return (double)(r >> 8) / 16777216.0; };
    for (int b = 0; b < B; ++b) {
      double* x = &x0[(size_t)b * 13];
      x[2] = 3.0; x[3] = 1.0;
      for (int k = 0; k < 3; ++k) { x[7 + k] = 8.0 * (uni() - 0.5); x[10 + k] = uni() - 0.5; }
      for (int j = 0; j < 4; ++j) w[(size_t)b * 4 + j] = 0.1 + 0.3 * uni();
      mpcq::fleet::pack(p, m.g, row.data());
      for (int f = 0; f < mpcq::fleet::NF; ++f) tab[(size_t)f * B + b] = row[f];
    }
    double *d_x0, *d_x, *d_w, *d_tab;
    CHECK(hipMalloc((void**)&d_x0, x0.size() * sizeof(double)));
    CHECK(hipMalloc((void**)&d_x, x0.size() * sizeof(double)));
    CHECK(hipMalloc((void**)&d_w, w.size() * sizeof(double)));
    CHECK(hipMalloc((void**)&d_tab, tab.size() * sizeof(double)));
    CHECK(hipMemcpy(d_x0, x0.data(), x0.size() * sizeof(double), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_w, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    mpcq::fleet::Args a;
    a.tab = d_tab; a.B = B; a.b0 = 0; a.n = B; a.g = m.g; a.period = 0; a.xs = d_x; a.w = d_w; a.n_sub = n_sub; a.sim_dt = sim_dt;
    std::vector<float> t_plant, t_fleet;
    for (int it = 0; it < warm + launches; ++it)
      for (int which = 0; which < 2; ++which) {
        CHECK(hipMemcpyAsync(d_x, d_x0, x0.size() * sizeof(double), hipMemcpyDeviceToDevice, s));
        CHECK(hipEventRecord(e0, s));
        if (which == 0) hipLaunchKernelGGL(mpcq::plant_kernel<double>, dim3((B + 63) / 64), dim3(64), 0, s, m, d_x, d_w, n_sub, sim_dt, B);
        else hipLaunchKernelGGL(mpcq::fleet::fleet_plant_kernel, dim3((B + 63) / 64), dim3(64), 0, s, a);
        CHECK(hipGetLastError());
        CHECK(hipEventRecord(e1, s));
        CHECK(hipEventSynchronize(e1));
        float ms = 0;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (it >= warm) (which == 0 ? t_plant : t_fleet).push_back(ms * 1e3f);
        if (it == warm) CHECK(hipMemcpy((which == 0 ? xa : xb).data(), d_x, x0.size() * sizeof(double), hipMemcpyDeviceToHost));
      }
    const bool same = std::memcmp(xa.data(), xb.data(), xa.size() * sizeof(double)) == 0;
    if (!same) {   // which state components differ, and by how much
      for (int k = 0; k < 13; ++k) {
        double d = 0;
        for (int q = 0; q < B; ++q) d = std::max(d, std::fabs(xa[(size_t)q * 13 + k] - xb[(size_t)q * 13 + k]));
        std::fprintf(stderr, "B %d n_sub %d component %d largest difference %.3e\n", B, n_sub, k, d);
      }
    }
    std::printf("{\"batch\": %d, \"n_sub\": %d, \"sim_dt\": %g, \"launches\": %d, \"wavefronts\": %d, \"plant_kernel_us\": {\"median\": %.3f, \"min\": %.3f}, "
                "\"fleet_plant_kernel_us\": {\"median\": %.3f, \"min\": %.3f}, \"default_plants_bit_identical\": %s}\n",
                B, n_sub, sim_dt, launches, (B + 63) / 64, median(t_plant), *std::min_element(t_plant.begin(), t_plant.end()), median(t_fleet),
                *std::min_element(t_fleet.begin(), t_fleet.end()), same ? "true" : "false");
    CHECK(hipFree(d_x0)); CHECK(hipFree(d_x)); CHECK(hipFree(d_w)); CHECK(hipFree(d_tab));
  }
  CHECK(hipEventDestroy(e0)); CHECK(hipEventDestroy(e1)); CHECK(hipStreamDestroy(s));
  return 0;
}

// mpcq_circle.hpp — device circle generator (mpcq_replan_circle, circle legs of a device mission).  Included from mpcq_api.hip after
// mpcq_replan.hpp.
//
// The three closed-form circle flights of the reference's TrajectoryGenerator (sample_circle_trajectory_acc_dec / sample_circle_trajectory /
// sample_circle_trajectory_accelerating) as trajectories.circle_trajectory states them on the host, one wavefront per quadrotor:
//  * the row count is numpy's len(arange(0, stop, dt)) = ceil(stop / dt) with `stop` formed by the reference's expression, operation for
//    operation, in double;
//  * the running sums w += acc dt and phi += w dt are sequential in the reference, and a rounding of the 6-decimal output can flip on the
//    last bit of phi: one lane accumulates them in row order, a chunk of CIRCLE_CHUNK rows at a time into LDS (no wavefront scan, which
//    would reassociate the sums);
//  * the per-row work -- sin / cos, p = r cos(phi) - r + start, v, the 6-decimal rounding of sample_install -- is spread over the 64 lanes;
//  * the install is slot_commit's.  A negative code returns before the first store to the slot.
// Floating-point contraction is off: the host forms every product and sum separately.
#pragma once

namespace mpcq {
namespace replan {

// flight kinds (include/mpcq.h MPCQ_CIRCLE_*)
constexpr int CIRCLE_ACC_DEC = 0, CIRCLE_CONSTANT = 1, CIRCLE_ACCELERATING = 2;
constexpr int CIRCLE_CHUNK = 128;   // rows per sequential pass; w and phi of a chunk live in Lds::R, which a circle does not use otherwise
static_assert(2 * CIRCLE_CHUNK <= MAXF * RW, "a chunk of w and phi must fit Lds::R");

// The circle flight of one quadrotor, by the wavefront that calls it: from p0 [3], radius `radius`, peak speed `v_max`; on DONE installed in
// slot b.  t_max: the duration of CIRCLE_ACCELERATING (not read otherwise).  Returns the MPCQ_REPLAN_* code (wave-uniform).  Starts with a
// barrier, so that a workgroup may plan one quadrotor after another in the same LDS.  Shared by circle_kernel (a host call) and
// mission_kernel (mpcq_mission.hpp, behind a period).
__device__ inline int plan_circle(Lds& S, double* traj, int Tmax, int* lens, int* idx, int* finished, int b, const double* p0, double radius, double v_max,
                                  int kind, double dt, double t_max) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x;
  __syncthreads();
  const double sx = p0[0], sy = p0[1], sz = p0[2];   // (every lane reads the same three values)
  if (!(__builtin_isfinite(sx) && __builtin_isfinite(sy) && __builtin_isfinite(sz) && __builtin_isfinite(radius) && __builtin_isfinite(v_max) &&
        radius > 0.0 && v_max > 0.0))
    return BAD_INPUT;
  const double pi = 3.141592653589793;
  const double w_max = v_max / radius;
  double acc = 0.0, t_mid = 0.0, stop;
  if (kind == CIRCLE_ACC_DEC) {
    acc = w_max * w_max / 2.0 / pi;
    t_mid = w_max / acc;
    stop = 2 * t_mid;
  } else if (kind == CIRCLE_CONSTANT) {
    stop = 2 * pi / w_max;
  } else {
    stop = t_max;
  }
  const double count = ceil(stop / dt);
  if (!(count >= 1.0)) return BAD_INPUT;   // (w_max under- or overflowed: no row, or not a number)
  if (count > (double)Tmax) return TOO_LONG;
  const int rows = (int)count;
  double* W = &S.R[0][0];
  double* PHI = W + CIRCLE_CHUNK;
  double* slot = traj + (size_t)b * Tmax * NX;
  double w = 0.0, phi = 0.0;   // the running sums (lane 0)
  for (int k0 = 0; k0 < rows; k0 += CIRCLE_CHUNK) {
    const int n = rows - k0 < CIRCLE_CHUNK ? rows - k0 : CIRCLE_CHUNK;
    if (kind == CIRCLE_ACCELERATING) {   // w is a closed form of the row number here; only phi is a running sum
      for (int j = lane; j < n; j += 64) {
        const double k = ((double)(k0 + j + 1) / (double)rows * 2) - 1;
        W[j] = (sin((k * 2 * pi + pi * 3 / 2) * 0.5) + 1) / 2 * w_max;
      }
      __syncthreads();
    }
    if (lane == 0)
      for (int j = 0; j < n; ++j) {
        if (kind == CIRCLE_ACC_DEC) {
          const double t = (k0 + j) * dt;
          w = w + (t < t_mid ? acc : -acc) * dt;
          W[j] = w;
        } else if (kind == CIRCLE_CONSTANT) {
          w = w_max;
          W[j] = w;
        } else {
          w = W[j];
        }
        phi = phi + w * dt;
        PHI[j] = phi;
      }
    __syncthreads();
    for (int j = lane; j < n; j += 64) {
      const double ph = PHI[j], wj = W[j], s = sin(ph), c = cos(ph);
      double row[NX];
      for (int i = 0; i < NX; ++i) row[i] = 0.0;
      row[3] = 1.0;
      const double p[3] = {radius * c - radius + sx, radius * s + sy, 0.0 + sz};
      const double v[2] = {-radius * wj * s, radius * wj * c};
      for (int a = 0; a < 3; ++a) row[a] = rint(p[a] * 1e6) / 1e6;
      for (int a = 0; a < 2; ++a) row[7 + a] = rint(v[a] * 1e6) / 1e6;
      for (int i = 0; i < NX; ++i) slot[(size_t)(k0 + j) * NX + i] = row[i];
    }
    __syncthreads();   // (the next chunk overwrites W and PHI)
  }
  slot_commit(S, traj, Tmax, b, rows, lens, idx, finished);
  return DONE;
}

// One workgroup (one wavefront) per quadrotor.  start: [B,3] or the plant state [B,13] (start_stride 13); radius, v_max: [B]; mask: [B] or
// NULL (the finished flags select).  code [B]: MPCQ_REPLAN_*.
__global__ __launch_bounds__(64) void circle_kernel(double* traj, int Tmax, int* lens, int* idx, int* finished, const double* start, int start_stride,
                                                    const double* radius, const double* v_max, int kind, double dt, double t_max, const int* mask,
                                                    int* code) {
  Lds& S = *reinterpret_cast<Lds*>(smem_raw);
  const int b = blockIdx.x;
  const bool sel = mask ? mask[b] != 0 : finished[b] != 0;
  int c = SKIPPED;
  if (sel) c = plan_circle(S, traj, Tmax, lens, idx, finished, b, start + (size_t)b * start_stride, radius[b], v_max[b], kind, dt, t_max);
  if (threadIdx.x == 0) code[b] = c;
}

}  // namespace replan
}  // namespace mpcq

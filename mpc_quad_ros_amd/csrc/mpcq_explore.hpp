// mpcq_explore.hpp — exploration on the device (mpcq_explore_start / _get / _stop): every quadrotor keeps the envelope of the body-frame
// velocities it has flown, and in the period a flight ends the limits of its next mission leg are set from that envelope by the
// reference's rule (src/Explorer.py:40-84, applied as src/explore_trajectories.py:59-125 applies it).  Included from mpcq_api.hip after
// mpcq_mission.hpp and mpcq_record.hpp; the step kernel, its state and mission_kernel are untouched.
//
//  * explore_kernel, one launch per period and range [b0, b0 + n): behind the step launch (and the recorder's row and the score, where
//    those run), in front of the plant launch and the mission launch.  The finished flag and the leg counter are final there, the
//    measurement is still the one the step solved from, and the mission launch of the same period reads the legs table this launch wrote.
//  * The sample of a period is v_body = R(q)^T v of that measurement, through record::v_body_axis (mpcq_record.hpp), the function
//    record_kernel's F_DRAG calls: the envelope is bit for bit the minimum and maximum of the recorded v_body rows.
//  * MPCQ_EXPLORE_LAST_FLIGHT: a period whose step used cursor 0 (idx - 1 == 0, the first period of a flight, as MPCQ_RECORD_SOLVER shows
//    it) restarts the envelope at its own sample -- the reference trains a fresh GP on every run.  MPCQ_EXPLORE_CUMULATIVE never restarts.
//  * A quadrotor is due when finished[b] != 0 && leg[b] < L; if leg_mask[b, leg[b]] is set the launch writes v_max and a_max of
//    legs[b, leg[b]] (kind and radius stay) and the triple (explored, v_max, a_max) into leg_limits[b, leg[b]].
// One lane per quadrotor: 13 doubles of the measurement, its rule and its envelope.  No LDS, no atomics; nothing a lane writes is read by
// another lane of the launch.
#pragma once

namespace mpcq {
namespace explore {

constexpr int BLOCK = 64;

struct Args {
  double* env;                     // [B,3,2]: min, max of v_body per axis (zeros while samples == 0)
  int64_t* samples;                // [B]
  const mpcq_explore_rule* rules;  // [B]
  const unsigned char* leg_mask;   // [B,L]
  mpcq_leg* legs;                  // [B,L]: the mission's table
  double* leg_limits;              // [B,L,3]: explored, v_max, a_max (NaN: not written)
  const int* leg;                  // [B]: the mission's leg counters
  const int *idx, *finished;       // [B]: the cursor behind the step's post phase, the finished flag
  const double* xmeas;             // [B,13]: the measurement the period's step solved from
  int L, b0, n;                    // the range [b0, b0 + n) of this launch
};

inline unsigned grid(int n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

// Explorer.calculate_explored_vmax (src/Explorer.py:51-63) over the axes of `axes` and calculate_velocity_to_explore (:40-48), then the
// clips of src/explore_trajectories.py:70-78.  env: min, max per axis.  out: explored, v_max, a_max.
__host__ __device__ inline void rule_apply(const double* env, const mpcq_explore_rule& r, double* out) {
  double explored = 0;
  bool first = true;
  for (int i = 0; i < 3; ++i) {
    if (!(r.axes >> i & 1)) continue;
    const double mn = env[2 * i], mx = env[2 * i + 1], amn = mn < 0 ? -mn : mn;
    double vabs = 0;
    if (mx > vabs) vabs = mx;
    if (amn > vabs) vabs = amn;
    if (first || vabs < explored) explored = vabs;   // (min(): the first of equal values)
    first = false;
  }
  const double next = explored + r.step;
  const double v = next < r.desired ? next : r.desired;
  out[0] = explored;
  out[1] = v > r.v_limit ? r.v_limit : v;
  out[2] = v > r.a_limit ? r.a_limit : v;
}

__global__ void __launch_bounds__(BLOCK) explore_kernel(const Args a) {
  const int t = blockIdx.x * BLOCK + threadIdx.x;
  if (t >= a.n) return;
  const int b = a.b0 + t;
  // ---- the period's sample (record_kernel, F_DRAG)
  double x[NX], vb[3];
#pragma unroll
  for (int k = 0; k < NX; ++k) x[k] = a.xmeas[(size_t)b * NX + k];
#pragma unroll
  for (int i = 0; i < 3; ++i) vb[i] = record::v_body_axis(x, i);
  // ---- the envelope
  const mpcq_explore_rule r = a.rules[b];
  const int64_t have = a.samples[b];
  const bool restart = have == 0 || (r.mode == MPCQ_EXPLORE_LAST_FLIGHT && a.idx[b] - 1 == 0);
  double env[6];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double mn = a.env[(size_t)b * 6 + 2 * i], mx = a.env[(size_t)b * 6 + 2 * i + 1];
    if (restart) mn = mx = vb[i];
    if (vb[i] < mn) mn = vb[i];
    if (vb[i] > mx) mx = vb[i];
    env[2 * i] = mn; env[2 * i + 1] = mx;
    a.env[(size_t)b * 6 + 2 * i] = mn; a.env[(size_t)b * 6 + 2 * i + 1] = mx;
  }
  a.samples[b] = restart ? 1 : have + 1;
  // ---- the limits of the leg the mission launch of this period is about to plan
  const int l = a.leg[b];
  if (a.finished[b] == 0 || l >= a.L || l < 0) return;
  const size_t at = (size_t)b * a.L + l;
  if (!a.leg_mask[at]) return;
  double out[3];
  rule_apply(env, r, out);
  a.legs[at].v_max = out[1];
  a.legs[at].a_max = out[2];
#pragma unroll
  for (int k = 0; k < 3; ++k) a.leg_limits[at * 3 + k] = out[k];
}

}  // namespace explore
}  // namespace mpcq

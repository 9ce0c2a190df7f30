// mpcq_sensor.hpp — the sensor (mpcq_sensor_start / _get / _sample / _stop): noise, bias, latency and dropout between the plant and the
// controller, per quadrotor.  Included from mpcq_api.hip only, after mpcq_kernels.hpp; the step kernel and its state are untouched -- the
// step takes its measurement by pointer, and while a sensor runs mpcq_sim_steps points it at this kernel's output.
//
//  * sensor_kernel runs in front of everything else a control period issues (sensor_launch, from EngineT::period) and once per
//    mpcq_sensor_sample.  One lane per quadrotor, blocks of one wavefront, arguments b0 / n / B as fleet_plant_kernel.  No LDS, no
//    atomics; nothing a lane writes is read by another lane.
//  * The table is field-major, tab[field * B + b], the ring component-major, ring[(slot * 13 + c) * B + b]: the 64 lanes of a
//    wavefront load and store 64 neighbouring doubles.  The plant state it reads and the measurement it delivers are [B,13] rows, the
//    layout the step kernel reads.
//  * Sensor period n, quadrotor b of global index i = index0 + b (DESIGN section 21 has the full text):
//      draws    Philox4x32-10, counter (n lo, n hi, i lo, c), key (seed lo, seed hi), c = 0..3.  A word w is u = (w + 0.5) 2^-32; calls
//               0..2 give the normals z[4c .. 4c + 3] by Box-Muller from the word pairs (0, 1) and (2, 3), word 0 of call 3 is u_drop.
//      sample   p, v, r: x + bias + sigma z with z[0:3], z[6:9], z[9:12]; attitude: q (x) the rotation vector bias_att + sigma_att z[3:6],
//               normalised.  A channel whose sigma and bias are all zero is copied, so an all-zero sensor is the identity bit for bit.
//      ring     the sample goes to slot (n - period0) mod depth.
//      deliver  the candidate is the sample of period max(n - delay, period0).  With n > period0 and (u_drop < p_drop or out_from <= n <
//               out_to) the period is dropped: the delivered measurement stays, age += 1.  Else delivered = candidate, age =
//               min(delay, n - period0).
//  * The draws depend on (seed, n, i) alone: not on the batch, the group of the launch or the order of launches.  Philox's 32 x 32 -> 64
//    products are plain C++ (the lane emulator compiles this file unchanged).  The calls a lane does not need are skipped: no sigma, no
//    normals; p_drop = 0, no call 3.
#pragma once

namespace mpcq {
namespace sensor {

// fields of the device table, [NF][B] doubles, in the order of mpcq_sensor; channel k (p, att, v, r) has sigma at F_SIGMA + 3 k and bias at
// F_BIAS + 3 k
constexpr int F_SIGMA = 0, F_BIAS = 12, F_PDROP = 24, NF = 25;
// the table of 64-bit integers, [NI][B]
constexpr int I_FROM = 0, I_TO = 1, NI = 2;
constexpr int MAX_DEPTH = 32;

// one quadrotor's row in the order of the table (host: mpcq_sensor_start)
inline void pack(const mpcq_sensor& s, double* row /*[NF]*/) {
  const double* sig[4] = {s.sigma_p, s.sigma_att, s.sigma_v, s.sigma_r};
  const double* bias[4] = {s.bias_p, s.bias_att, s.bias_v, s.bias_r};
  for (int k = 0; k < 4; ++k)
    for (int i = 0; i < 3; ++i) { row[F_SIGMA + 3 * k + i] = sig[k][i]; row[F_BIAS + 3 * k + i] = bias[k][i]; }
  row[F_PDROP] = s.p_drop;
}

struct Args {
  const double* tab;       // [NF][B]
  const long long* win;    // [NI][B]: out_from, out_to
  int* ints;               // delay [B] | age [B]
  int B;                   // the engine's batch: stride of a field
  int b0, n;               // the range [b0, b0 + n) of this launch
  int depth;
  long long period, since, index0;   // the sensor period n, n - period0 >= 0, the global index of quadrotor 0
  unsigned key0, key1;     // the seed's halves
  const double* x;         // [B][13] the true plant state
  double* ring;            // [depth][13][B] | the delivered measurement [B][13]
};
// (a handful of arguments fewer -- age and the delivered measurement at fixed places behind delay and the ring -- is what keeps the
// kernel's scalar registers from spilling: the constants of log and sincos take most of them)

// Philox4x32-10 (Salmon et al., SC'11): ten rounds, the key bumped between them
__host__ __device__ inline void philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned* w /*[4]*/) {
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0; c1 = (unsigned)p1; c2 = n2; c3 = (unsigned)p0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}
// a word as a uniform in (0, 1): exact in double, never 0 or 1
__host__ __device__ inline double uniform(unsigned w) { return ((double)w + 0.5) * (1.0 / 4294967296.0); }
// two normals from two words
__host__ __device__ inline void box_muller(unsigned wa, unsigned wb, double* z /*[2]*/) {
  const double rho = sqrt(-2.0 * log(uniform(wa))), phi = 6.283185307179586 * uniform(wb);
  double sn, cs;
  sincos(phi, &sn, &cs);   // (one argument reduction for both)
  z[0] = rho * cs;
  z[1] = rho * sn;
}

// The value as it is, in a vector register, behind an empty statement the compiler does not see through.  The constants of log and sincos
// take most of the scalar registers while the draws are made; what the kernel needs behind them -- where the lane reads and writes, which
// calls it makes -- is formed in front, per lane, and pinned with this, so that no kernel argument and no lane mask has to stay in a
// scalar register over the draws (they spilled from there: 22 SGPRs with everything unrolled and held as the compiler liked).
template <typename V> __device__ inline void pin(V& v) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(v));
#else
  (void)v;
#endif
}

__global__ void __launch_bounds__(64) sensor_kernel(const Args a) {
  const int lane = blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= a.n) return;
  const size_t b = (size_t)a.b0 + lane, B = (size_t)a.B;
  // ---- where this lane reads and writes, and what it has to do
  const double* t = a.tab + b;   // field f of this quadrotor: t[f * B]
  const double* xb = a.x + b * NX;
  double* out = a.ring + (size_t)a.depth * NX * B + b * NX;
  int* age = a.ints + B + b;
  const long long j = a.since;   // periods since the first
  const int delay = a.ints[b];
  const long long back = delay < j ? delay : j;   // the candidate is the sample of period n - back (back <= depth - 1)
  double* ring_w = a.ring + (size_t)(j % a.depth) * NX * B + b;            // slot (n - period0) mod depth, component c at ring_w[c * B]
  const double* ring_r = a.ring + (size_t)((j - back) % a.depth) * NX * B + b;
  size_t stride = B;
  double sig[12];
  bool noisy = false;
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    sig[k] = t[(F_SIGMA + k) * B];
    noisy = noisy || sig[k] != 0.0;
  }
  const double p_drop = t[F_PDROP * B];
  const bool outage = a.win[I_FROM * B + b] <= a.period && a.period < a.win[I_TO * B + b];
  // bit 0: the normals (calls 0..2); bit 1: u_drop (call 3); bit 2: an outage period; bit 3: the candidate comes from the ring
  int need = (noisy ? 1 : 0) | (j > 0 && p_drop > 0.0 ? 2 : 0) | (j > 0 && outage ? 4 : 0) | (back > 0 ? 8 : 0);
  const unsigned long long i = (unsigned long long)(a.index0 + (long long)b), n = (unsigned long long)a.period;
  unsigned n_lo = (unsigned)n, n_hi = (unsigned)(n >> 32), i_lo = (unsigned)i, k0 = a.key0, k1 = a.key1, back_i = (unsigned)back;
  pin(t); pin(xb); pin(out); pin(age); pin(ring_w); pin(ring_r); pin(stride); pin(n_lo); pin(n_hi); pin(i_lo); pin(k0); pin(k1); pin(back_i);
  // ---- draws.  One copy of Philox and of Box-Muller in the code, run up to four and six times; c and h are uniform over the wavefront
  // and the selects keep z in registers.
  double z[12], u_drop = 1.0;
#pragma unroll
  for (int k = 0; k < 12; ++k) z[k] = 0.0;
#pragma unroll 1
  for (unsigned c = 0; c < 4; ++c) {
    pin(need);
    if (!(need & (c < 3 ? 1 : 2))) continue;
    unsigned w[4];
    philox(n_lo, n_hi, i_lo, c, k0, k1, w);
    if (c == 3) { u_drop = uniform(w[0]); continue; }
#pragma unroll 1
    for (unsigned h = 0; h < 2; ++h) {
      double zz[2];
      box_muller(h ? w[2] : w[0], h ? w[3] : w[1], zz);
#pragma unroll
      for (int k = 0; k < 12; ++k) z[k] = (unsigned)(k >> 1) == 2 * c + h ? zz[k & 1] : z[k];
    }
  }
  pin(need);
  // ---- sample
  double bias[12], x[NX], m[NX];
  bool on[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    on[k] = false;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      bias[3 * k + i] = t[(F_BIAS + 3 * k + i) * stride];
      on[k] = on[k] || sig[3 * k + i] != 0.0 || bias[3 * k + i] != 0.0;
    }
  }
#pragma unroll
  for (int k = 0; k < NX; ++k) m[k] = x[k] = xb[k];
  if (on[0]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) m[k] = x[k] + bias[k] + sig[k] * z[k];
  }
  if (on[1]) {
    double th[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) th[k] = bias[3 + k] + sig[3 + k] * z[3 + k];
    const double ang = sqrt(th[0] * th[0] + th[1] * th[1] + th[2] * th[2]);
    double d[4] = {1.0, 0.0, 0.0, 0.0};
    if (ang != 0.0) {
      double sh, ch;
      sincos(0.5 * ang, &sh, &ch);
      const double sn = sh / ang;
      d[0] = ch; d[1] = sn * th[0]; d[2] = sn * th[1]; d[3] = sn * th[2];
    }
    const double *q = x + 3;
    double r[4];
    r[0] = q[0] * d[0] - q[1] * d[1] - q[2] * d[2] - q[3] * d[3];
    r[1] = q[0] * d[1] + q[1] * d[0] + q[2] * d[3] - q[3] * d[2];
    r[2] = q[0] * d[2] - q[1] * d[3] + q[2] * d[0] + q[3] * d[1];
    r[3] = q[0] * d[3] + q[1] * d[2] - q[2] * d[1] + q[3] * d[0];
    const double nrm = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3]);
#pragma unroll
    for (int k = 0; k < 4; ++k) m[3 + k] = r[k] / nrm;
  }
  if (on[2]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) m[7 + k] = x[7 + k] + bias[6 + k] + sig[6 + k] * z[6 + k];
  }
  if (on[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) m[10 + k] = x[10 + k] + bias[9 + k] + sig[9 + k] * z[9 + k];
  }
  // ---- ring
#pragma unroll
  for (int k = 0; k < NX; ++k) ring_w[k * stride] = m[k];
  // ---- deliver.  (u_drop is 1 where call 3 was not made: p_drop = 0, or the first period, which is never dropped)
  if (u_drop < p_drop || (need & 4)) { *age += 1; return; }
  if (need & 8) {   // (not the slot written above)
#pragma unroll
    for (int k = 0; k < NX; ++k) m[k] = ring_r[k * stride];
  }
#pragma unroll
  for (int k = 0; k < NX; ++k) out[k] = m[k];
  *age = (int)back_i;
}

}  // namespace sensor
}  // namespace mpcq

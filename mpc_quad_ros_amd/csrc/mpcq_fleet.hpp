// mpcq_fleet.hpp — the fleet (mpcq_fleet_set / _get / _stop): every quadrotor its own plant.  Included from mpcq_api.hip only, after
// mpcq_kernels.hpp; the step kernel, its state and plant_kernel are untouched.
//
//  * fleet_plant_kernel takes the place of plant_kernel in a period (fleet_launch, from EngineT::plant_launch) while a fleet is set: behind the
//    recorder's row and the score, in front of the mission launch.  Same mapping: one lane per quadrotor, blocks of one wavefront.
//  * The table lives on the device field-major, tab[field * B + b]: the 64 lanes of a wavefront load 64 neighbouring doubles per field
//    (one mpcq_plant as an array of structs would put the lanes 264 bytes apart).  A launch over the group [b0, b0 + n) indexes it with
//    field * B + b0 + lane.  What the integration needs as a quotient (1 / mass, 1 / J, f_d / mass, t_d / J, payload_mass g / mass) is in
//    the table as that quotient, formed once on the host (pack): no division in the kernel.
//  * A lane loads its row into registers once, in front of the substep loop; no LDS.  The disturbance window is decided there too:
//    outside [d_from, d_to) the lane integrates with f_d / mass = t_d / J = 0.
//  * The derivative is plant_eval of mpcq_kernels.hpp -- a template over its model type -- on a per-lane model, with the reference's
//    extras around it (src/quad.py:344-377): u * rotor_functionality in front; payload, rotated f_d / mass and t_d / J behind.  With
//    functionality 1, payload 0 and no disturbance every extra is an exact * 1.0 or + 0.0, so a row that restates the engine's plant
//    integrates bit for bit as plant_kernel does (a derivative that is -0.0 may come out as +0.0: equal as numbers).
//  * That identity needs plant_eval's own operations to be contracted into multiply-adds here exactly as in plant_kernel.  The compiler
//    fuses across statements and, where a sum of two products can be fused either way (a b + c d as fma(a, b, c d) or fma(c, d, a b): another
//    product is rounded), its choice depends on the code around the expression.  Three things keep it the same: `opaque` ends the expression
//    at plant_eval's results, so the additions behind them are not merged into the chains that formed them; the extras rotate with a matrix
//    of their own, formed from opaque copies of the quaternion, so that no term of plant_eval gains a further use; and fleet_rk4 is
//    plant_rk4 statement for statement (the clip inside, the same declarations and loops).  With a loop of another shape around the same
//    plant_eval, the body-velocity row R[0] v[0] + R[3] v[1] came out fused the other way and a default fleet differed from the shared
//    plant by 2.7e-13 after 8 closed-loop periods on the MI355X.  tests/test_fleet.py (defaults are the identity) holds this on the device.
//    It is tied to the fusion choices of the compiler at hand: fleet_rk4 has to follow any change of plant_rk4 by hand, and after a change of
//    toolchain that case may fail without the arithmetic being wrong -- tools/fleet_contraction_check.py (run by tests/test_fleet.py on the
//    built object, no GPU) then says which expression is contracted differently.
#pragma once

namespace mpcq {
namespace fleet {

// fields of the device table, [NF][B] doubles
constexpr int F_TMAX = 0, F_IMASS = 1, F_AERO = 2, F_RDRAG = 3 /*3*/, F_XF = 6 /*4*/, F_YF = 10 /*4*/, F_ZL = 14 /*4*/, F_J = 18 /*3*/, F_IJ = 21 /*3*/,
              F_FUN = 24 /*4*/, F_PAY = 28 /* payload_mass g / mass */, F_FDM = 29 /*3: f_d / mass*/, F_TDJ = 32 /*3: t_d / J*/,
              F_FROM = 35, F_TO = 36 /* the window, as doubles (exact for int32) */, NF = 37;

// one quadrotor's row in the order of the table (host: mpcq_fleet_set)
inline void pack(const mpcq_plant& p, double g, double* row /*[NF]*/) {
  row[F_TMAX] = p.max_thrust; row[F_IMASS] = 1.0 / p.mass; row[F_AERO] = p.aero_drag;
  for (int i = 0; i < 3; ++i) {
    row[F_RDRAG + i] = p.rotor_drag[i]; row[F_J + i] = p.J[i]; row[F_IJ + i] = 1.0 / p.J[i];
    row[F_FDM + i] = p.f_d[i] / p.mass; row[F_TDJ + i] = p.t_d[i] / p.J[i];
  }
  for (int j = 0; j < 4; ++j) {
    row[F_XF + j] = p.x_f[j]; row[F_YF + j] = p.y_f[j]; row[F_ZL + j] = p.z_l_tau[j]; row[F_FUN + j] = p.rotor_functionality[j];
  }
  row[F_PAY] = p.payload_mass * g / p.mass;
  row[F_FROM] = (double)p.d_from; row[F_TO] = (double)p.d_to;
}

// The value as it is, behind an empty statement the compiler does not see through: arithmetic in front of it and arithmetic behind it
// are never fused into one multiply-add.  (Host builds of the kernels do not contract at all.)
__device__ inline void opaque(double& v) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(v));
#else
  (void)v;
#endif
}

// what plant_eval reads of its model, per lane
struct LaneModel {
  double tmax, imass, aero_drag, rotor_drag[3], g, xf[4], yf[4], zl[4], J[3], iJ[3];
};

struct Args {
  const double* tab;   // [NF][B]
  int B;               // the engine's batch: stride of a field
  int b0, n;           // the range [b0, b0 + n) of this launch
  double g;            // the engine's
  double period;       // the fleet period of this update
  double* xs;          // [B][13] plant states
  const double* w;     // [B][4] controls
  int n_sub;
  double sim_dt;
};

struct Extras { double fdm[3], tdj[3], pay; };
// plant_eval with the reference's extras behind it
template <typename M>
__device__ inline void fleet_eval(const M& m, const Extras& e, const double* x, const double* u, double* f) {
  plant_eval(m, x, u, f);
#pragma unroll
  for (int i = 7; i < NX; ++i) opaque(f[i]);
  double qo[4] = {x[3], x[4], x[5], x[6]}, R[9];
#pragma unroll
  for (int i = 0; i < 4; ++i) opaque(qo[i]);   // (a rotation matrix of its own: sharing plant_eval's would give its terms further uses)
  rotmat(qo, R);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    f[7 + i] += R[3 * i] * e.fdm[0] + R[3 * i + 1] * e.fdm[1] + R[3 * i + 2] * e.fdm[2];
    f[10 + i] += e.tdj[i];
  }
  f[9] -= e.pay;
}
// plant_rk4 of mpcq_kernels.hpp, statement for statement, around fleet_eval
template <typename M>
MPCQ_PHASE void fleet_rk4(const M& m, const Extras& e, double* x, const double* uin, double dt) {
  double u[4], k[NX], xt[NX], acc[NX];
#pragma unroll
  for (int j = 0; j < 4; ++j) u[j] = tmin(1.0, tmax(0.0, uin[j]));
#pragma unroll
  for (int i = 0; i < NX; ++i) { xt[i] = x[i]; acc[i] = 0; }
  MPCQ_RK_LOOP
  for (int s = 0; s < 4; ++s) {
    fleet_eval(m, e, xt, u, k);
    const double wa = (s == 0 || s == 3) ? 1.0 : 2.0, hc = s == 2 ? dt : dt / 2;
#pragma unroll
    for (int i = 0; i < NX; ++i) { acc[i] += wa * k[i]; xt[i] = x[i] + hc * k[i]; }
  }
#pragma unroll
  for (int i = 0; i < NX; ++i) x[i] = x[i] + dt / 6 * acc[i];
}

// n_sub RK4 substeps (Quadrotor3D.update -> one_step_forward, src/quad.py:166-190, 234-253) of every quadrotor's own plant
__global__ void __launch_bounds__(64) fleet_plant_kernel(const Args a) {
  const int lane = blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= a.n) return;
  const size_t b = (size_t)a.b0 + lane, B = (size_t)a.B;
  const double* t = a.tab + b;   // field f of this quadrotor: t[f * B]
  LaneModel m;
  m.tmax = t[F_TMAX * B]; m.imass = t[F_IMASS * B]; m.aero_drag = t[F_AERO * B]; m.g = a.g;
  double fdm[3], tdj[3], ue[NU], x[NX];
  const bool gust = t[F_FROM * B] <= a.period && a.period < t[F_TO * B];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    m.rotor_drag[i] = t[(F_RDRAG + i) * B]; m.J[i] = t[(F_J + i) * B]; m.iJ[i] = t[(F_IJ + i) * B];
    const double f = t[(F_FDM + i) * B], q = t[(F_TDJ + i) * B];
    fdm[i] = gust ? f : 0.0; tdj[i] = gust ? q : 0.0;
  }
  const double pay = t[F_PAY * B];
#pragma unroll
  for (int j = 0; j < NU; ++j) {
    m.xf[j] = t[(F_XF + j) * B]; m.yf[j] = t[(F_YF + j) * B]; m.zl[j] = t[(F_ZL + j) * B];
    // update() clips the input (:242-247), f_vel / f_rate scale it by the rotor's functionality (:344, :371)
    ue[j] = tmin(1.0, tmax(0.0, a.w[b * NU + j])) * t[(F_FUN + j) * B];
  }
#pragma unroll
  for (int k = 0; k < NX; ++k) x[k] = a.xs[b * NX + k];
  const double dt = a.sim_dt;
  Extras e;
  for (int i = 0; i < 3; ++i) { e.fdm[i] = fdm[i]; e.tdj[i] = tdj[i]; }
  e.pay = pay;
  for (int s = 0; s < a.n_sub; ++s) fleet_rk4(m, e, x, ue, dt);
#pragma unroll
  for (int k = 0; k < NX; ++k) a.xs[b * NX + k] = x[k];
}

}  // namespace fleet
}  // namespace mpcq

// mpcq_record.hpp — the flight recorder (mpcq_record_start / _get): one row per selected quadrotor and recorded period, written by
// launches placed around the period's step launch.  Included from mpcq_api.hip only; the step kernel and its state are untouched.
//
//  * record_snapshot_kernel, in front of the step launch (MPCQ_RECORD_DRAG only): x_pred_prev and has_prev the step starts from,
//    which its post phase overwrites.
//  * record_kernel, behind the step launch and in front of any plant launch: every requested field of the period, read from the
//    device state the step left.  Each field is stored period-major, [capacity][count][width], so one launch writes one contiguous
//    slab per field; lanes run over the flattened (quadrotor, element) index of the slab -- 64 consecutive lanes store 64
//    consecutive values -- and read the per-quadrotor records contiguously (the reference row is the only gather).
// Blocks of one wavefront, no LDS, no atomics; the write position (row) is host bookkeeping.
#pragma once

namespace mpcq {
namespace record {

// fields in bit order of include/mpcq.h MPCQ_RECORD_*: x_odom, x_ref, w, x_pred, cost, drag, rgp_mu, rgp_C, solver
constexpr int NF = 9, F_XODOM = 0, F_XREF = 1, F_W = 2, F_XPRED = 3, F_COST = 4, F_DRAG = 5, F_MU = 6, F_C = 7, F_SOLVER = 8;
constexpr int SNAP = NX + 1;   // snapshot row: x_pred_prev (13), has_prev
__host__ __device__ inline int width(int f, int nb) {
  switch (f) {
    case F_XODOM: case F_XREF: case F_XPRED: return NX;
    case F_W: return NU;
    case F_COST: return 1;
    case F_DRAG: return 6;
    case F_MU: return 3 * nb;
    case F_C: return 3 * nb * nb;
    default: return 4;
  }
}

// Component i of v_body = R(q)^T v of the state x [13] (rotmat's R, column i).  The one place the recorder's v_body is computed, and
// the exploration's sample with it (mpcq_explore.hpp): the envelope of an exploration is bit for bit the minimum and maximum of the
// recorded rows only if both kernels round alike, and left to itself the compiler fuses these products and sums into multiply-adds
// differently from kernel to kernel (and, inside record_kernel, from component to component).  So contraction is off here: every
// operation is rounded on its own, whatever the code around the call.
__device__ inline double v_body_axis(const double* x, int i) {
#pragma clang fp contract(off)
  const double qw = x[3], qx = x[4], qy = x[5], qz = x[6];
  double r0, r1, r2;   // R[i], R[3 + i], R[6 + i]
  if (i == 0) { r0 = 1 - 2 * (qy * qy + qz * qz); r1 = 2 * (qx * qy + qw * qz); r2 = 2 * (qx * qz - qw * qy); }
  else if (i == 1) { r0 = 2 * (qx * qy - qw * qz); r1 = 1 - 2 * (qx * qx + qz * qz); r2 = 2 * (qy * qz + qw * qx); }
  else { r0 = 2 * (qx * qz + qw * qy); r1 = 2 * (qy * qz - qw * qx); r2 = 1 - 2 * (qx * qx + qy * qy); }
  return r0 * x[7] + r1 * x[8] + r2 * x[9];
}

// What a row is read from: the device state a step left (and, for MPCQ_RECORD_DRAG, the snapshot taken in front of it)
template <typename TQ>
struct Source {
  const double* snap;  // [count][SNAP]
  const double* xmeas; const double* w; const double* xpred; const double* cost; const double* traj;
  const int* tlen; const int* idx; const int* finished; const int* status; const int* qp_iter;
  const TQ* mu; const TQ* C;
  int Tmax, N, skip, nb;
  double dt_pred;
};
template <typename TQ>
struct Args : Source<TQ> {
  const int* sel;      // selection, sorted [count]
  int j0, n;           // the part of the selection this launch covers: [j0, j0 + n)
  int count;           // selection size (row stride of a slab)
  int row;             // write position
  int blk[NF + 1];     // first block of each field; blk[NF] = blocks of the launch (a field not recorded has no blocks)
  double* out[NF - 1]; // double fields [capacity][count][width]
  int* solver;         // [capacity][count][4] int32
};

__global__ void __launch_bounds__(64) record_snapshot_kernel(const int* sel, int j0, int n, const double* xpp, const int* has_prev, double* snap) {
  const long t = (long)blockIdx.x * 64 + threadIdx.x;
  if (t >= (long)n * SNAP) return;
  const int jl = (int)(t / SNAP), k = (int)(t - (long)jl * SNAP), j = j0 + jl, b = sel[j];
  snap[(size_t)j * SNAP + k] = k < NX ? xpp[(size_t)b * NX + k] : (double)has_prev[b];
}

// Element e of double field f (not F_SOLVER) of the period the step has just left, for quadrotor b at place j of the selection.  The one
// place a row value is made: record_kernel and the black box's row kernel (mpcq_blackbox.hpp) both store what this returns.
template <typename TQ>
__device__ inline double row_value(const Source<TQ>& a, int f, int e, int j, int b) {
  switch (f) {
    case F_XODOM: return a.xmeas[(size_t)b * NX + e];
    case F_XREF: {   // row 0 of the chunk the step used: the post phase has advanced the cursor by one
      const int idx = a.idx[b] - 1, len = a.tlen[b];
      const long r = chunk_row(0, chunk_have(len, idx, a.N, a.skip), idx, a.skip, len);
      return a.traj[((size_t)b * a.Tmax + r) * NX + e];
    }
    case F_W: return a.w[(size_t)b * NU + e];
    case F_XPRED: return a.xpred[(size_t)b * NX + e];
    case F_COST: return a.cost[b];
    case F_DRAG: {   // compute_a_drag of the post phase (mpcq_kernels.hpp, step_kernel section 4) against the snapshot
      double x[NX], xq[NX];
      const double* sn = a.snap + (size_t)j * SNAP;
      const bool hp = sn[NX] != 0.0;
#pragma unroll
      for (int k = 0; k < NX; ++k) { x[k] = a.xmeas[(size_t)b * NX + k]; xq[k] = hp ? sn[k] : x[k]; }
      const int c = e < 3 ? e : e - 3;
      const double vb = v_body_axis(x, c), vp = v_body_axis(xq, c);
      return e < 3 ? vb : (vb - vp) / a.dt_pred;
    }
    case F_MU: return (double)a.mu[(size_t)b * 3 * a.nb + e];
    default: return (double)a.C[(size_t)b * 3 * a.nb * a.nb + e];
  }
}
// Element e of F_SOLVER: status, qp_iter, the cursor the step used, the finished flag after the step
template <typename TQ>
__device__ inline int solver_value(const Source<TQ>& a, int e, int b) {
  if (e == 0) return a.status[b];
  if (e == 1) return a.qp_iter[b];
  if (e == 2) return a.idx[b] - 1;
  return a.finished[b];
}
// The lane's place in a launch over a.blk: field f, element e, place j of the selection.  false: the lane is beyond its field's slab.
template <typename TQ>
__device__ inline bool lane_place(const Args<TQ>& a, int bx, int lane, int& f, int& e, int& j) {
  int first = 0;   // the field of this block (block-uniform; constant indices keep the argument arrays out of scratch)
  f = 0;
#pragma unroll
  for (int k = 1; k < NF; ++k)
    if (bx >= a.blk[k]) { f = k; first = a.blk[k]; }
  const int W = width(f, a.nb);
  const long t = (long)(bx - first) * 64 + lane;
  if (t >= (long)a.n * W) return false;
  const int jl = (int)(t / W);
  e = (int)(t - (long)jl * W); j = a.j0 + jl;
  return true;
}
// The lane's value into row a.row of its field's slab
template <typename TQ>
__device__ inline void put_row(const Args<TQ>& a, int f, int e, int j) {
  const int b = a.sel[j];
  const size_t o = ((size_t)a.row * a.count + j) * width(f, a.nb) + e;
  if (f == F_SOLVER) { a.solver[o] = solver_value(a, e, b); return; }
  double* dst = a.out[0];
#pragma unroll
  for (int k = 1; k < NF - 1; ++k)
    if (f == k) dst = a.out[k];
  dst[o] = row_value(a, f, e, j, b);
}

template <typename TQ>
__global__ void __launch_bounds__(64) record_kernel(const Args<TQ> a) {
  int f, e, j;
  if (lane_place(a, (int)blockIdx.x, (int)threadIdx.x, f, e, j)) put_row(a, f, e, j);
}

}  // namespace record
}  // namespace mpcq

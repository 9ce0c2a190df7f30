// mpcq_blackbox.hpp — the incident recorder (mpcq_blackbox_start / _get): every watched quadrotor owns a ring of D = pre + 1 + post of the
// flight recorder's rows, overwritten every period until a rule of its own, judged on the device, has fired and `post` more periods have
// passed.  Included from mpcq_api.hip only, after mpcq_record.hpp; the step kernel and its state are untouched.
//
//  * record::record_snapshot_kernel, in front of the step launch (MPCQ_RECORD_DRAG only), into the black box's own [count][SNAP] buffer.
//  * row_kernel, behind the recorder's row: record_kernel's lanes and record_kernel's values (record::lane_place / put_row) into ring slot
//    p % D of every quadrotor that is not frozen.  The layout is the recorder's, [D][count][width] per field.
//  * judge_kernel, behind row_kernel on the same stream: one lane per quadrotor judges the rule on the period's values and moves the
//    state armed -> fired -> frozen.
//    Two launches, not one kernel in two phases: the lanes that write a quadrotor's row run over the flattened (quadrotor, element) index
//    of every field's slab, so they sit in as many blocks as there are fields (and, for the wide RGP fields, more), while the state
//    changes once per quadrotor.  A rendezvous orders the lanes of one block only; the launch boundary orders them all, and the row lanes
//    see the state from before the period's update by construction.
//  * gather_kernel (read-out): the rings of a caller-chosen subset in time order, left-aligned, [n][D][width]; rows beyond a quadrotor's
//    count are NaN (-1 for the solver ints).  Only this staging block travels to the host.
//  * init_kernel: the state of the selected quadrotors at start and rearm.
// Blocks of one wavefront, no LDS, no atomics; the slot and the period number are host bookkeeping passed by value.
#pragma once

namespace mpcq {
namespace blackbox {

constexpr int ARMED = 0, FIRED = 1, FROZEN = 2;
// causes, in bit order of include/mpcq.h MPCQ_BB_*
constexpr int C_STATUS = 1, C_FALLBACK = 2, C_NONFINITE = 4, C_ERR_POS = 8, C_SPEED = 16, C_TILT = 32, C_COST = 64, C_ALL = 127;

// Per-quadrotor state of the selection (sorted order), [count] each
struct State {
  int *state, *cause, *left;
  long long *fired, *first;   // fired_period (-1: not fired); the first period whose row the ring holds
};

template <typename TQ>
struct RowArgs : record::Args<TQ> {   // (row: the ring slot)
  const int* state;
};

struct JudgeArgs {
  const int* sel;      // selection, sorted [count]
  int j0, n;           // the part of the selection this launch covers: [j0, j0 + n)
  const mpcq_blackbox_rule* rules;   // [count], sorted order
  State st;
  long long period;
  int post;
  const double* xmeas; const double* w; const double* cost; const double* traj;
  const int* tlen; const int* idx; const int* status; const int* qp_iter;
  int Tmax, N, skip;
};

// The cause word of one period: x the measurement [13], ref the reference row [13], w the control [4].  Contraction is off for the reason
// record::v_body_axis gives: the host restates these expressions on recorded rows (params.blackbox_causes) and has to meet them exactly.
__device__ inline int judge(const mpcq_blackbox_rule& r, const double* x, const double* ref, const double* w, double cost, int status, int qp_iter) {
#pragma clang fp contract(off)
  int c = 0;
  if ((status & r.status_mask) != 0) c |= C_STATUS;
  if (qp_iter / 1000 % 10 != 0) c |= C_FALLBACK;
  bool finite = __builtin_isfinite(cost);
#pragma unroll
  for (int k = 0; k < NX; ++k) finite = finite && __builtin_isfinite(x[k]);
#pragma unroll
  for (int k = 0; k < NU; ++k) finite = finite && __builtin_isfinite(w[k]);
  if (!finite) c |= C_NONFINITE;
  const double dx = x[0] - ref[0], dy = x[1] - ref[1], dz = x[2] - ref[2];
  if (((dx * dx + dy * dy) + dz * dz) > r.err_pos * r.err_pos) c |= C_ERR_POS;
  const double vx = x[7], vy = x[8], vz = x[9];
  if (((vx * vx + vy * vy) + vz * vz) > r.speed * r.speed) c |= C_SPEED;
  const double qx = x[4], qy = x[5];
  if (1 - 2 * (qx * qx + qy * qy) < r.tilt_cos) c |= C_TILT;
  if (cost > r.cost) c |= C_COST;
  return c & r.causes;
}

template <typename TQ>
__global__ void __launch_bounds__(64) row_kernel(const RowArgs<TQ> a) {
  int f, e, j;
  if (!record::lane_place(a, (int)blockIdx.x, (int)threadIdx.x, f, e, j)) return;
  if (a.state[j] == FROZEN) return;
  record::put_row(a, f, e, j);
}

__global__ void __launch_bounds__(64) judge_kernel(const JudgeArgs a) {
  const long t = (long)blockIdx.x * 64 + threadIdx.x;
  if (t >= a.n) return;
  const int j = a.j0 + (int)t, b = a.sel[j];
  int s = a.st.state[j];
  if (s == FROZEN) return;
  int left = a.st.left[j];
  if (s == FIRED) --left;
  else {
    const int i = a.idx[b] - 1, len = a.tlen[b];   // the post phase has advanced the cursor by one
    const long r = chunk_row(0, chunk_have(len, i, a.N, a.skip), i, a.skip, len);   // record_kernel's x_ref
    const int c = judge(a.rules[j], a.xmeas + (size_t)b * NX, a.traj + ((size_t)b * a.Tmax + r) * NX, a.w + (size_t)b * NU, a.cost[b], a.status[b],
                        a.qp_iter[b]);
    if (c == 0) return;
    a.st.fired[j] = a.period; a.st.cause[j] = c;
    s = FIRED; left = a.post;
  }
  a.st.state[j] = left == 0 ? FROZEN : s;
  a.st.left[j] = left;
}

// Armed with an empty ring that begins with period `first`: place j of the selection where mask [count] is non-zero (nullptr: everywhere)
__global__ void __launch_bounds__(64) init_kernel(State st, const int* mask, int count, long long first) {
  const long j = (long)blockIdx.x * 64 + threadIdx.x;
  if (j >= count || (mask && !mask[j])) return;
  st.state[j] = ARMED; st.cause[j] = 0; st.left[j] = 0;
  st.fired[j] = -1; st.first[j] = first;
}

// Rings in time order: out [n][D][W]; item i is place which[i] of the selection, its rows the periods p0[i] .. p0[i] + rows[i] - 1 (ring slot
// = period % D), the rest `fill`.  src [D][count][W].
template <typename V>
__global__ void __launch_bounds__(64) gather_kernel(const V* src, const int* which, const long long* p0, const int* rows, long total, int D, int W, int count,
                                                    V fill, V* out) {
  const long t = (long)blockIdx.x * 64 + threadIdx.x;
  if (t >= total) return;
  const long per = (long)D * W;
  const int i = (int)(t / per);
  const long u = t - (long)i * per;
  const int r = (int)(u / W), e = (int)(u - (long)r * W);
  V v = fill;
  if (r < rows[i]) v = src[((size_t)((p0[i] + r) % D) * count + which[i]) * W + e];
  out[t] = v;
}

}  // namespace blackbox
}  // namespace mpcq

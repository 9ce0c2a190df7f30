// mpcq_score.hpp — the flight scoreboard (mpcq_score_start / _get): one launch behind every period folds that period into the row of the
// flight the quadrotor is flying, so a sweep that flies as one batch is read as [B, flights, 16] doubles at its end.  Included from
// mpcq_api.hip after mpcq_record.hpp; the step kernel and its state are untouched.
//
//  * score_kernel, behind the recorder's row launch and in front of the plant and mission launches: it reads what record_kernel reads
//    (the measurement the step solved from, idx - 1 = the cursor the step used, tlen, traj, status, qp_iter, cost, finished).
//  * A slot row is 16 doubles, one 128-byte line.  A quadrotor is one 16-lane row of a wavefront and lane k owns field k of the row: the
//    row reads and writes exactly one line of the table, and the inputs (three records of the quadrotor, six entries each of the
//    measurement and of the reference row) are same-address loads within the row.  Four quadrotors per wavefront.
//  * A flight begins with a period whose step used cursor 0: if the current slot already holds a period the row moves to the next slot.
//    No install path knows about the score.  A quadrotor out of slots counts the period in overflow[b] and writes nothing else.
//  * What one lane writes another reads (cur[b], and fields 0 and 8 of the current slot as its "holds a period" mark), so the kernel is
//    two phases around one rendezvous: every load of shared state in front of it, every store behind it.
// Blocks of one wavefront, no LDS, no atomics; the period number is host bookkeeping.
#pragma once

namespace mpcq {
namespace score {

constexpr int W = 16;   // MPCQ_SCORE_WIDTH
// Threads per block of score_kernel: exactly one wavefront.  Lane 0 of a row stores cur[b], which the other 15 lanes of the row load, and
// lanes 0 and 8 store the fields every lane loads as the slot's "holds a period" mark; all of a quadrotor's lanes sit in one wavefront
// (W divides 64), the loads are in front of the rendezvous and the stores behind it.  A block of several wavefronts would still keep a row
// inside one of them, but review the two phases before changing this.
constexpr int BLOCK = 64;
static_assert(BLOCK == 64 && BLOCK % W == 0, "score_kernel: one wavefront per block, whole rows per wavefront");
// fields of a row, in the order of include/mpcq.h
constexpr int F_STEPS = 0, F_SUM_EPOS2 = 1, F_SUM_EVEL2 = 2, F_MAX_EPOS2 = 3, F_SUM_RMS_POS = 4, F_MAX_V2 = 5, F_MAX_VREF2 = 6, F_SUM_COST = 7,
              F_TAIL_STEPS = 8, F_BAD_STATUS = 9, F_FALLBACKS = 10, F_FACTORISATIONS = 11, F_FIRST_PERIOD = 12, F_LAST_PERIOD = 13, F_ROWS = 14,
              F_FINISHED = 15;
__host__ __device__ inline double start_value(int k) { return k == F_FIRST_PERIOD || k == F_LAST_PERIOD ? -1.0 : 0.0; }

struct Args {
  double* table;       // [B][F][W]
  int *cur, *used, *overflow;   // [B]: current slot (<= F), slots holding a period, periods that found no slot
  int F, tail_rows;
  int b0, n;           // the range [b0, b0 + n) of this launch
  double period;       // period number since mpcq_score_start / mpcq_score_clear
  const double* xmeas; const double* cost; const double* traj;
  const int* tlen; const int* idx; const int* finished; const int* status; const int* qp_iter;
  int Tmax, N, skip;
};

inline unsigned grid(long lanes) { return (unsigned)((lanes + BLOCK - 1) / BLOCK); }

// table, cur, used and overflow of the quadrotors [0, B) to their start values
__global__ void __launch_bounds__(BLOCK) score_init_kernel(double* table, int* ints, long B, int F) {
  const long t = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (t < B * F * W) table[t] = start_value((int)(t & (W - 1)));
  if (t < 3 * B) ints[t] = 0;
}

__global__ void __launch_bounds__(BLOCK) score_kernel(const Args a) {
  const long t = (long)blockIdx.x * BLOCK + threadIdx.x;
  const int q = (int)(t >> 4), k = (int)(threadIdx.x & (W - 1));
  const bool live = q < a.n;   // (the last wavefront of a range may carry idle rows: they take part in the rendezvous only)
  const int b = a.b0 + (live ? q : 0);
  // ---- phase 1: everything this row shares between its lanes is read
  const int i = a.idx[b] - 1, len = a.tlen[b];   // the post phase has advanced the cursor by one
  int c = a.cur[b];
  const bool moved = i == 0 && c < a.F && a.table[((size_t)b * a.F + c) * W + F_STEPS] + a.table[((size_t)b * a.F + c) * W + F_TAIL_STEPS] > 0;
  if (moved) ++c;
  const bool slot = c < a.F;
  double* row = a.table + ((size_t)b * a.F + (slot ? c : 0)) * W;
  double v = slot ? row[k] : 0.0;
  __syncthreads();
  // ---- phase 2: lane k folds the period into field k
  if (!live) return;
  if (k == 0) {
    if (moved) a.cur[b] = c;
    if (slot) a.used[b] = c + 1;
    else a.overflow[b] = a.overflow[b] + 1;
  }
  if (!slot) return;
  const bool tail = i >= len - a.tail_rows;
  const long r = chunk_row(0, chunk_have(len, i, a.N, a.skip), i, a.skip, len);   // row 0 of the chunk the step used: record_kernel's x_ref
  const double* x = a.xmeas + (size_t)b * NX;
  const double* ref = a.traj + ((size_t)b * a.Tmax + r) * NX;
  double ep = 0, ev = 0, v2 = 0, vr2 = 0;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double dp = x[j] - ref[j], dv = x[7 + j] - ref[7 + j];
    ep += dp * dp; ev += dv * dv;
    v2 += x[7 + j] * x[7 + j]; vr2 += ref[7 + j] * ref[7 + j];
  }
  const int it = a.qp_iter[b];
  bool write = !tail;   // fields 0..7: the flight without its tail
  switch (k) {
    case F_STEPS: v += 1.0; break;
    case F_SUM_EPOS2: v += ep; break;
    case F_SUM_EVEL2: v += ev; break;
    case F_MAX_EPOS2: v = ep > v ? ep : v; break;
    case F_SUM_RMS_POS: v += sqrt(ep / 3.0); break;
    case F_MAX_V2: v = v2 > v ? v2 : v; break;
    case F_MAX_VREF2: v = vr2 > v ? vr2 : v; break;
    case F_SUM_COST: v += a.cost[b]; break;
    case F_TAIL_STEPS: v += 1.0; write = tail; break;
    case F_BAD_STATUS: v += a.status[b] != 0 ? 1.0 : 0.0; write = true; break;
    case F_FALLBACKS: v += it / 1000 % 10 != 0 ? 1.0 : 0.0; write = true; break;
    case F_FACTORISATIONS: v += (double)(it % 1000); write = true; break;
    case F_FIRST_PERIOD: v = v < 0 ? a.period : v; write = true; break;
    case F_LAST_PERIOD: v = a.period; write = true; break;
    case F_ROWS: v = (double)len; write = true; break;
    default: v = (v != 0 || a.finished[b] != 0) ? 1.0 : 0.0; write = true;
  }
  if (write) row[k] = v;
}

}  // namespace score
}  // namespace mpcq
